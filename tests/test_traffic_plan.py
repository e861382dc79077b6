"""The host runtime's launch planning (gr-liquiddsp_amd/csrc/fx_traffic.h: what the last collected block held, the grids and
optional launches of the next block's tail, what such a plan leaves for fxrx_collect) as a small host-only driver
(tests/cpp/traffic_check.cpp) built with g++ under AddressSanitizer and UndefinedBehaviorSanitizer.  Properties, at 256 and 8
CUs and with 1000 and 40 chain slots: a first block launches everything at capacity (the Reed-Solomon instance at
min(slots, 64)); a block like the last one leaves nothing to collect, clean or not; one quantity beyond the plan yields
exactly its reason; the Reed-Solomon grid shrinks to zero and the trellis kernels stay for kTrellisHold plans."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-g"]
ENV = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")


def test_traffic_plan_properties(tmp_path):
    exe = str(tmp_path / "traffic_check")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-I/opt/rocm/include", "-D__HIP_PLATFORM_AMD__"] + SAN +
                          ["-o", exe, os.path.join(ROOT, "tests", "cpp", "traffic_check.cpp")])
    r = subprocess.run([exe], capture_output=True, text=True, env=ENV, timeout=60)
    assert r.returncode == 0, (r.stdout[-4000:], r.stderr[-4000:])
    assert "checks, 0 failures" in r.stdout and "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr
