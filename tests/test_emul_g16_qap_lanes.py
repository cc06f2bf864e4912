"""The lane-per-proof QAP passes of the Groth16 prover (libzkp_amd/csrc/g16_steps.h: g16_qap_pass_single / _pair / _triple in the launch
order of g16_qap_lane_schedule, both pass shapes) on the host, no GPU: tests/emul/emul_g16_qap_lanes.cpp runs every task of every pass for both circuits
(m = 512 and m = 1024) on three rows -- 64-bit extreme values, membership sets of 1 and 64 elements -- and compares all m - 1 digit rows
of h word for word with g16_qap_proof's.  The program is built under AddressSanitizer and UndefinedBehaviorSanitizer with buffers of
exactly the prover's sizes, so an access outside [3][m][9][rows] or the digit rows ends it."""
import subprocess


def test_every_pass_of_both_circuits_matches_g16_qap_proof_under_sanitizers():
    import __graft_entry__ as ge
    exe = ge.build_emul_qap_lanes()
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    lines = r.stdout.strip().splitlines()
    assert lines[-1] == "ok", lines
    assert lines[:4] == [
        "kind 0, passes of up to 2 stages: m = 512, 15 launches, 35 polynomial passes, 3 rows x 511 digit rows of h identical",
        "kind 1, passes of up to 2 stages: m = 1024, 15 launches, 35 polynomial passes, 3 rows x 1023 digit rows of h identical",
        "kind 0, passes of up to 3 stages: m = 512, 9 launches, 21 polynomial passes, 3 rows x 511 digit rows of h identical",
        "kind 1, passes of up to 3 stages: m = 1024, 12 launches, 28 polynomial passes, 3 rows x 1023 digit rows of h identical"], lines
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-4000:]
