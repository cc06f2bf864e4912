"""The key points that the Groth16 sums A and B1 share (libzkp_amd/csrc/g16_share.h), on the CPU: the committed keys' 110 shared
variables, the windows the A / B1 launch loses, the three slot lists A' | S | B1' read back from the step lists of several chunkings
(every (point, scalar row, window) of A and of B1 exactly once), the degenerate keys, and one launch walked on the host against
double-and-add.  The slots come from the key loader's own plan (g16_share.h), whose other decisions are checked here too: lists C and
G2, scalar rows, windows, base order, the point counts the radix is chosen from, the offset corrections of every sum, and the
proving-key reader's rules (g16_keyblob.h).  tests/emul/emul_g16_shared_points.cpp is a program of its own: it is run once as built, and once built with the host
sanitizers."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "emul", "emul_g16_shared_points.cpp")
KEYS = [os.path.join(ROOT, "tests", "golden", name) for name in ("equality_mimc_pk.bin", "membership_mimc_pk.bin")]
CIRCUITS = ("equality", "membership")
CHECKS = (["shared_count_%s" % c for c in CIRCUITS]
          + ["%s_%s_w%d" % (what, c, w) for what in ("windows_fall", "switch_off_is_parent", "each_term_once") for c in CIRCUITS for w in (13, 8)]
          + ["no_coincidence_is_parent_layout", "infinity_pair_ignored", "different_index_ignored", "negation_not_shared",
             "msm_walk_w8", "msm_walk_w13", "msm_walk_w14_uneven"]
          # the loader's whole plan (g16_share.h): lists C and G2, scalar rows and windows, base order, window sums, with the switch on and off
          + ["%s_%s_w%d" % (what, c, w) for what in ("lists_c_g2", "rows_windows", "slot_is_base", "window_sums") for c in CIRCUITS for w in (13, 8)]
          + ["point_counts_%s_%s" % (c, sw) for c in CIRCUITS for sw in ("shared", "switch_off")] + ["table_points_%s" % c for c in CIRCUITS]
          + ["offset_counts_%s" % c for c in CIRCUITS + ("synthetic",)]
          + ["reader_accepts_committed_key", "reader_truncated", "reader_trailing_bytes", "reader_a_query_length", "reader_delta_g1_infinity"])


def build_and_run(tmp, name, flags):
    exe = str(tmp / name)
    subprocess.check_call(["g++", "-std=c++17"] + flags + ["-o", exe, SRC])
    return subprocess.run([exe] + KEYS, capture_output=True, text=True)


def verdicts(stdout):
    out = {}
    for line in stdout.splitlines():
        word, name = line.split()[:2]
        out[name] = (word, line)
    return out


@pytest.fixture(scope="module")
def run(tmp_path_factory):
    r = build_and_run(tmp_path_factory.mktemp("emul_g16_shared"), "emul_g16_shared_points", ["-O2"])
    return r.returncode, verdicts(r.stdout)


@pytest.mark.parametrize("check", CHECKS)
def test_check(run, check):
    assert check in run[1], "the program printed no verdict for this check"
    assert run[1][check][0] == "ok", run[1][check][1]


def test_every_verdict_is_listed_and_the_exit_status_counts_failures(run):
    assert sorted(run[1]) == sorted(CHECKS)
    assert run[0] == sum(1 for v in run[1].values() if v[0] != "ok")


def test_the_keys_lose_110_points_tables(run):
    """110 x nwin windows: 2 200 of 11 059 (equality) and of 13 294 (membership) at radix 2^13."""
    assert run[1]["windows_fall_equality_w13"][1].endswith("11059 -> 8859")
    assert run[1]["windows_fall_membership_w13"][1].endswith("13294 -> 11094")
    assert run[1]["windows_fall_equality_w8"][1].endswith("17695 -> 14175")


def test_under_the_host_sanitizers(tmp_path):
    r = build_and_run(tmp_path, "emul_g16_shared_points_san", ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"])
    assert r.returncode == 0 and "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-2000:]
    assert all(v[0] == "ok" for v in verdicts(r.stdout).values()) and len(verdicts(r.stdout)) == len(CHECKS)
