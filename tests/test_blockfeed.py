"""The block feeder under flexframesync_execute and qdetector_cccf_execute (gr-liquiddsp_amd/csrc/fx_blockfeed.h: the ring of page-locked
buffers, submit / collect / drop / restart, all-or-nothing resizing, context replacement) as a host-only driver
(tests/cpp/blockfeed_check.cpp) linked against fakes of the eleven fxrx_* functions the header uses, built with g++ under
AddressSanitizer and UndefinedBehaviorSanitizer with leak detection on.  Samples carry their index; the fake context records every
block submitted, refuses more than `depth` in flight, checks at collect that no buffer was refilled while in flight, and fails the k-th
submit, collect or allocation.  Checked at depths 1, 2, 3, 15, block lengths 1, 7, 4096 and feed sizes 1, 256, 97: every sample is
submitted exactly once and in order or lies in a failed block, and the missing ones are exactly the failed block (submit) or all
blocks in flight (collect); a failed submit is followed by one reset after everything in flight was collected; errors counts each
failure once and stderr speaks at failures 1, 2, 4, 8, 16 of 20; a resize that fails at any of its depth + 1 allocations leaves ring,
block, cur, fill and the buffered samples alone and counts one error, frees match allocations; a failed context replacement keeps
the old context undestroyed, a good one destroys it once; flush on an empty feeder submits nothing.  The same driver runs once more
without sanitizers at -O2."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "blockfeed_check.cpp")
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-g"]
ENV = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")


def _run(tmp_path, name, flags):
    exe = str(tmp_path / name)
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror"] + flags + ["-o", exe, SRC])
    r = subprocess.run([exe], capture_output=True, text=True, env=ENV, timeout=120)
    assert r.returncode == 0, (r.stdout[-4000:], r.stderr[-4000:])
    assert "checks, 0 failures" in r.stdout and "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr and "LeakSanitizer" not in r.stderr


def test_block_feeder_under_sanitizers(tmp_path):
    _run(tmp_path, "blockfeed_check", ["-O1"] + SAN)


def test_block_feeder_without_sanitizers(tmp_path):
    _run(tmp_path, "blockfeed_check_o2", ["-O2"])
