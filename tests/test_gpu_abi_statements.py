"""The statement verifier called from C++ through the headers alone (tests/abi/abi_call_statements.cpp): the ops and the output of
zkp_hip_process_batch go straight into zkp_stmt_verify and, in device memory, into zkp_stmt_verify_device, without Python in the call path."""
import os
import subprocess

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_cpp_program_verifies_a_proved_batch_against_its_ops():
    import __graft_entry__ as ge
    exe = ge.build_abi_statements_caller()
    r = subprocess.run([exe, os.path.join(ROOT, "tests", "golden")], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-4000:]
    assert "abi_call_statements ok: 3 symbols" in r.stdout
