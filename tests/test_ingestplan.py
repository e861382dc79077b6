"""The input routes of a block (gr-liquiddsp_amd/csrc/fx_ingestplan.h: which of six ways the new samples of a stream take into the
float buffer the kernels read) as a small host-only driver (tests/cpp/ingestplan_check.cpp) built with g++ under AddressSanitizer
and UndefinedBehaviorSanitizer.  Checked, at the default limits and at limits that are no multiple of a sample, zero and huge:
every row of the header's table (format x device / page-locked / pageable); both sides of each size limit (the most samples within
it: a kernel reads page-locked memory; one sample more, the first beyond limit + 1 bytes: the copy engines); a page-locked float
pointer off its 8-byte alignment goes to the copy engines, integer IQ at any multiple of its sample size does not; a stream
without new samples gets no route."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-g"]
ENV = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")


def test_ingest_routes(tmp_path):
    exe = str(tmp_path / "ingestplan_check")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Werror"] + SAN + ["-o", exe, os.path.join(ROOT, "tests", "cpp", "ingestplan_check.cpp")])
    r = subprocess.run([exe], capture_output=True, text=True, env=ENV, timeout=60)
    assert r.returncode == 0, (r.stdout[-4000:], r.stderr[-4000:])
    assert "checks, 0 failures" in r.stdout and "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr
