"""The stand-alone host programs of tests/tools (each with its own main), built
with g++ and run on the CPU for the tests that pin the kernel-selection policy
and the C ABI's refusals.  The compiler flags and the list of kernel objects
live in one file, tests/tools/asan.mk, and are asked of it here.  Nothing is
launched on a device and nothing sanitised is loaded into Python.
"""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "cuda-dct-idct_amd")
TOOLS = os.path.join(ROOT, "tests", "tools")


def asan_mk(name):
    """A variable of tests/tools/asan.mk, as make expands it."""
    r = subprocess.run(["make", "-s", "-f", os.path.join(TOOLS, "asan.mk"), "-f", "-", "print"],
                       input="print:\n\t@echo $(%s)\n" % name, capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr
    return r.stdout.split()


def _build_and_run(name, tmp_path, flags, inputs, build_timeout, run_timeout, env=None):
    exe = str(tmp_path / name)
    b = subprocess.run(["g++"] + flags + [os.path.join(TOOLS, name + ".cpp")] + inputs + ["-o", exe],
                       capture_output=True, text=True, timeout=build_timeout)
    assert b.returncode == 0, b.stdout + b.stderr
    r = subprocess.run([exe], capture_output=True, text=True, timeout=run_timeout, env=env)
    assert r.returncode == 0, r.stdout + r.stderr
    assert name + ": ok" in r.stdout
    return r


def policy_check(name, tmp_path):
    """tests/tools/<name>.cpp, a table of hpdct_policy.hpp's choices: headers only, no library, warnings are
    errors, ASan + UBSan."""
    _build_and_run(name, tmp_path, ["-Wall", "-Werror"] + asan_mk("CXXF"), [], 300, 60)


def sanitised_check(name, tmp_path, kernel_object):
    """tests/tools/<name>.cpp with the C ABI's host sources (asan.mk's HOST list) under asan.mk's ASan + UBSan flags
    and the library's kernel objects linked as they are (host registration stubs only); kernel_object names one
    that must be among them."""
    kobj = asan_mk("KOBJ")
    want = [line.split(":=")[1].split() for line in open(os.path.join(PKG, "Makefile")) if line.startswith("KOBJ")][0]
    assert len(kobj) == len(want) and any(o.endswith(kernel_object) for o in kobj), \
        "library objects not built (__graft_entry__.build())"
    r = _build_and_run(name, tmp_path, asan_mk("CXXF"),
                       [os.path.join(PKG, "csrc", h + ".cpp") for h in asan_mk("HOST")] + kobj +
                       ["-L/opt/rocm/lib", "-Wl,-rpath,/opt/rocm/lib", "-lamdhip64", "-lpthread", "-lm"], 600, 120,
                       env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:halt_on_error=1",
                                UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1"))
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr
