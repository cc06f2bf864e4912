"""The mixed verifier called from C++ through the headers alone (tests/abi/abi_call_verify.cpp): what zkp_hip_process_batch wrote goes
straight back into zkp_hip_verify_envelopes and, in device memory, into zkp_hip_verify_envelopes_device, without Python in the call path."""
import os
import subprocess

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_cpp_program_calls_the_mixed_verifier():
    import __graft_entry__ as ge
    exe = ge.build_abi_verify_caller()
    r = subprocess.run([exe, os.path.join(ROOT, "tests", "golden")], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-4000:]
    assert "abi_call_verify ok: 2 symbols" in r.stdout
