"""The frame format's code rules as the kernels and the host share them (gr-liquiddsp_amd/csrc/fx_fecdims.h: coded lengths,
puncturing rows, coded bits in front of a trellis step) against two independent statements: tests/ref_decode.py's own
length rules, and a count of the ones in the first t columns of the reference's puncturing matrices.  The header is
compiled into a small host-only driver (tests/cpp/fecdims_check.cpp) with g++ under AddressSanitizer and
UndefinedBehaviorSanitizer, which prints every value; every line must agree."""
import os
import subprocess

import ref_decode as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-g"]
ENV = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
NS = list(range(701)) + [65535 + 4]


def bits_before(fs, t):
    """ones in the first t columns of the scheme's puncturing matrix, the columns repeating with its period"""
    a, b = R.PUNCTURE[fs]
    return sum(a[c % len(a)] + b[c % len(b)] for c in range(t))


def bits_before_closed(fs, t):
    """the same count without the loop: whole periods, then the columns of the one begun"""
    a, b = R.PUNCTURE[fs]
    p = len(a)
    return (t // p) * (sum(a) + sum(b)) + sum(a[:t % p]) + sum(b[:t % p])


def test_fecdims_header_against_reference_rules(tmp_path):
    exe = str(tmp_path / "fecdims_check")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-I/opt/rocm/include", "-D__HIP_PLATFORM_AMD__"] + SAN +
                          ["-o", exe, os.path.join(ROOT, "tests", "cpp", "fecdims_check.cpp")])
    r = subprocess.run([exe], capture_output=True, text=True, env=ENV, timeout=600)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr
    got = {}
    for line in r.stdout.splitlines():
        f = line.split()
        got[(f[0], int(f[1]), int(f[2]))] = [int(x) for x in f[3:]]
    for t in range(64):                                       # the closed form is the loop's count
        assert all(bits_before_closed(fs, t) == bits_before(fs, t) for fs in R.CONV)
    want = {}
    for fs in R.ALL_FEC:
        for n in NS:
            want[("L", fs, n)] = [R.fec_enc_len(fs, n)]
    for fs in R.CONV:
        a, b = R.PUNCTURE[fs]
        want[("M", fs, len(a))] = [sum(v << c for c, v in enumerate(a)), sum(v << c for c, v in enumerate(b))]
        for t in range(41):
            want[("B", fs, t)] = [bits_before_closed(fs, t)]
        for n in NS:
            want[("E", fs, n)] = [bits_before_closed(fs, 8 * n + 6)]
    assert sorted(got) == sorted(want)
    bad = [(k, got[k], want[k]) for k in want if got[k] != want[k]]
    assert not bad, bad[:10]
    # packet_dims chains the same rule twice behind the check's bytes
    for check in (R.CRC_NONE, R.CRC_8, R.CRC_16, R.CRC_24, R.CRC_32):
        for fec0, fec1 in ((R.FEC_V27P34, R.FEC_H128), (R.FEC_RS, R.FEC_V27), (R.FEC_SD39, R.FEC_NONE)):
            k = 100 + R.crc_len(check)
            l0 = got[("L", fec0, k)][0]
            assert tuple(R.packet_dims(100, check, fec0, fec1)) == (k, l0, got[("L", fec1, l0)][0])
