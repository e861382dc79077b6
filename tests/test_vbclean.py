"""The batch Viterbi path's codeword check (gr-liquiddsp_amd/csrc/fx_vbclean.h: the rate-1/2 K = 7 code inverted word by word,
re-encoded and compared) against the encoder, as a small host-only driver (tests/cpp/vbclean_check.cpp) built with g++
under AddressSanitizer and UndefinedBehaviorSanitizer: clean encodings of every length 1 .. 2048 bytes are accepted with their
message, bit errors and nonzero tails rejected, padding bits ignored."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-g"]
ENV = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")


def test_vbclean_check_against_encoder(tmp_path):
    exe = str(tmp_path / "vbclean_check")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-I/opt/rocm/include", "-D__HIP_PLATFORM_AMD__"] + SAN +
                          ["-o", exe, os.path.join(ROOT, "tests", "cpp", "vbclean_check.cpp")])
    r = subprocess.run([exe], capture_output=True, text=True, env=ENV, timeout=600)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    assert "2048 lengths, 0 failures" in r.stdout and "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr
