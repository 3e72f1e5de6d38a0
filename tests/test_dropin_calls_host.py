"""The C++ drop-in (putslam_amd/csrc/dropin/putslam_dropin.cpp) is an argument-marshalling layer: what it owes its callers is the same
C ABI calls with the same arguments in the same order, the same lines on std::cerr / std::cout and the same results handed back.
tests/cpp/test_dropin_calls.cpp drives every entry point except matchXYZLadder -- accepted calls, every refusal, the C ABI call
failing -- over tests/cpp/capi_recorder.cpp, a recording stand-in of the C ABI, as one plain program: no GPU.  Its transcript is
compared byte for byte with tests/golden/dropin_calls_parent.txt, recorded before the drop-in's helpers were consolidated (the file's
two-line header names the commit) and never regenerated from later code."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "dropin_calls_parent.txt")


def build_program(exe, extra=()):
    d = os.path.join(ROOT, "putslam_amd", "csrc", "dropin")
    cpp = os.path.join(ROOT, "tests", "cpp")
    # (-lamdhip64: matchXYZLadder's device block is the only user of the HIP runtime, and nothing the driver calls reaches it)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-pthread", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", "-I",
                           os.path.join(ROOT, "include"), "-I", d, *extra, os.path.join(d, "putslam_dropin.cpp"),
                           os.path.join(cpp, "capi_recorder.cpp"), os.path.join(cpp, "test_dropin_calls.cpp"), "-o", exe,
                           "-L/opt/rocm/lib", "-lamdhip64", "-Wl,-rpath,/opt/rocm/lib"])


def transcript(exe):
    run = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert run.returncode == 0, run.stdout[-2000:]
    return run.stdout


def test_dropin_makes_the_parents_calls(tmp_path):
    exe = str(tmp_path / "test_dropin_calls")
    build_program(exe)
    got = transcript(exe)
    with open(GOLDEN) as f:
        header, want = f.readline(), f.read()
    assert header.startswith("# recorded at commit "), header
    want = want.split("\n", 1)[1]  # (the header's second line)
    assert "\n== done\n" in got  # (the singletons' and the thread's destructors still write after it)
    if got != want:
        g, w = got.splitlines(), want.splitlines()
        at = next((i for i, (a, b) in enumerate(zip(g, w)) if a != b), min(len(g), len(w)))
        raise AssertionError("transcript line %d differs (of %d, golden %d):\n  got    %s\n  golden %s" %
                             (at + 1, len(g), len(w), g[at] if at < len(g) else "<end>", w[at] if at < len(w) else "<end>"))
