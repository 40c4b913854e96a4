"""CPU-only: the host's side of Gauss-Newton relocalisation (x-slam_amd/host/gn_host.hpp): the six seeded poses against their definition,
the damped 6 x 6 step it shares with newton_host.hpp, and the batched loop RelocalizeGaussNewtonBatch and RelocalizeNewtonBatch both run,
driven with chunks of 2 by a fake launch and step (tests/cxx/gn_selftest.cpp)."""
import os
import subprocess


def test_gn_host_code_holds_and_runs_clean_under_sanitizers(tmp_path):
    """tests/cxx/gn_selftest.cpp compiled with -fsanitize=address,undefined -fno-sanitize-recover and run, as tests/test_newton_cpu.py does
    for newton_host.hpp: a stand-alone program, nothing loaded into Python."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = str(tmp_path / "gn_selftest")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-ffp-contract=off", "-Wall", "-Werror",
           "-I" + os.path.join(root, "x-slam_amd", "host"), os.path.join(root, "tests", "cxx", "gn_selftest.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1"))
    assert r.returncode == 0 and "all checks held" in r.stdout, (r.stdout[-2000:], r.stderr[-3000:])
