"""The kernel-selection policy (cuda-dct-idct_amd/csrc/hpdct_policy.hpp) pinned
on the CPU.  Every mapping computes the same bits, so the GPU tests cannot tell
which kernel a call chose; tests/tools/policy_check.cpp asserts, for a table of
calls, the kernel family, variant bits, workgroup size, residency cap and grid.
Host code only: g++ with the flags tests/tools/asan.mk builds the host sources
with, no device and no library needed.
"""
import os
import shutil

import host_programs


def test_policy_table(tmp_path):
    # the only pin of the policy: a missing toolchain is a failure, not a skip
    assert shutil.which("g++") is not None, "g++ not found: the policy table cannot be checked"
    assert os.path.isdir("/opt/rocm/include"), "ROCm headers not found: the policy table cannot be checked"
    host_programs.policy_check("policy_check", tmp_path)
