"""Soft-decision header decoding (fxrx_config.soft_header) without a GPU: the numpy reference of tests/ref_header_soft.py against
the header encoder and against brute force, and the new entry points of libfxrx.so and the liquid shim."""
import os
import subprocess

import numpy as np
import pytest

import ref_decode as R
import ref_header_soft as H

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_reference_decodes_clean_headers():
    rng = np.random.RandomState(11)
    hdr = rng.randint(0, 256, (200, 20)).astype(np.uint8)
    tr = {}
    enc = np.stack([H.header_encode(h, tr) for h in hdr])
    assert enc.shape == (200, 54) and len(tr["cw0"]) == 27 and len(tr["cw1"]) == 54
    for got, ok in (H.decode_soft(H.hard_as_soft(enc)), H.decode_hard(enc)):
        assert (got == hdr).all() and ok.all()
    # mild noise on the soft values changes nothing
    noisy = np.clip(H.hard_as_soft(enc).astype(int) + rng.randint(-100, 101, (200, 432)), 0, 255)
    got, ok = H.decode_soft(noisy)
    assert (got == hdr).all() and ok.all()
    # one header through ref_decode's own packet chain
    assert R.packet_decode(enc[0], 20, R.CRC_32, R.FEC_SD72, R.FEC_H84) == (hdr[0].tobytes(), 1)


def test_crc_rows_match_ref_decode():
    rng = np.random.RandomState(3)
    msg = rng.randint(0, 256, (50, 20)).astype(np.uint8)
    assert [int(k) for k in H.crc32_rows(msg)] == [R.crc_key(R.CRC_32, m) for m in msg]


def _exhaustive(s):
    """the ML rule spelled out: cost of every message with plain integers, first minimum"""
    best, arg = None, None
    for d in range(16):
        c = int(R.code_table(R.FEC_H84)[2][d])
        cost = sum((255 - int(s[b])) if (c >> (7 - b)) & 1 else int(s[b]) for b in range(8))
        if best is None or cost < best:
            best, arg = cost, d
    return arg, best


def test_ml_stage_matches_exhaustive_search_with_ties():
    rng = np.random.RandomState(5)
    words = [rng.randint(0, 256, 8) for _ in range(3000)]
    words += [np.full(8, v) for v in (0, 1, 126, 127, 128, 129, 254, 255)]
    # forced ties: two codewords a, b at distance 4, the bits they share at 0 / 255, the four others with costs under a that
    # sum to 510 (= 4 x 255 / 2): a and b then cost the same
    tab = R.code_table(R.FEC_H84)[2]
    ties = 0
    while ties < 2000:
        a, b = rng.randint(0, 16, 2)
        ca, cb = int(tab[a]), int(tab[b])
        diff = [k for k in range(8) if ((ca ^ cb) >> (7 - k)) & 1]
        if len(diff) != 4:
            continue
        s = np.array([255 * ((ca >> (7 - k)) & 1) for k in range(8)])
        c1, c3 = rng.randint(0, 256, 2)
        for k, c in zip(diff, (c1, 255 - c1, c3, 255 - c3)):
            s[k] = 255 - c if (ca >> (7 - k)) & 1 else c
        words.append(s)
        ties += 1
    W = np.array(words)
    got_d, got_c = H.h84_ml(W)
    n_tied = 0
    for w, d, c in zip(W, got_d, got_c):
        ed, ec = _exhaustive(w)
        assert (d, c) == (ed, ec), w
        costs = [sum((255 - int(w[b])) if (int(tab[m]) >> (7 - b)) & 1 else int(w[b]) for b in range(8)) for m in range(16)]
        n_tied += costs.count(ec) > 1
    assert n_tied >= 2000                                          # the tie rule was exercised


def test_soft_on_hard_values_is_hard_decoding_for_every_word():
    r = np.arange(256)
    d_soft, cost = H.h84_ml(R.bits_of_words(r, 8).reshape(256, 8) * 255)
    d_hard, dist = R.nearest_codeword(R.FEC_H84, r)
    assert (d_soft == d_hard).all() and (cost == 255 * dist).all()
    # and whole headers: random received words, hard chain vs soft chain on 0 / 255
    rng = np.random.RandomState(9)
    enc = rng.randint(0, 256, (300, 54)).astype(np.uint8)
    a, va = H.decode_hard(enc)
    b, vb = H.decode_soft(H.hard_as_soft(enc))
    assert (a == b).all() and (va == vb).all()


def test_library_exports_the_soft_header_entry_points(fx):
    L = fx.lib()
    for name in ("flexframesync_decode_header_soft", "flexframesync_decode_payload_soft", "fxrx_debug_header_decode"):
        assert hasattr(L, name)
    assert "soft_header" in dict(fx._ffi.Config._fields_)
    # without a handle the setters report failure; the config field sits behind soft_decision
    assert L.flexframesync_decode_header_soft(None, 1) == -1 and L.flexframesync_decode_payload_soft(None, 1) == -1
    names = [n for n, _ in fx._ffi.Config._fields_]
    assert names.index("soft_header") == names.index("soft_decision") + 1


def test_detector_mode_refuses_soft_header(fx):
    L = fx.lib()
    cfg = fx._ffi.Config(0, 1, 1, 0.0, 0, 0, 0, 0, 1)
    assert not L.fxrx_create(cfg)
    if L.fxrx_device_count() > 0:
        assert b"soft_header" in L.fxrx_last_error()


@pytest.mark.parametrize("lang", ["c", "c++"])
def test_liquid_shim_compiles_calls_to_both_names(fx, tmp_path, lang):
    """include/liquid/liquid.h declares flexframesync_decode_header_soft / _payload_soft: a caller compiles, links against
    libfxrx.so alone and gets -1 for a NULL handle."""
    fx.lib()
    src = tmp_path / ("use.c" if lang == "c" else "use.cpp")
    src.write_text("#include <liquid/liquid.h>\n#include <stdio.h>\n"
                   "int main(void) { flexframesync q = 0; int a = flexframesync_decode_header_soft(q, 1);\n"
                   "  int b = flexframesync_decode_payload_soft(q, 0); printf(\"%d %d\\n\", a, b); return (a == -1 && b == -1) ? 0 : 1; }\n")
    exe = str(tmp_path / "use")
    lib = os.path.dirname(fx.LIB_PATH)
    cc = ["gcc", "-std=c11"] if lang == "c" else ["g++", "-std=c++11"]
    subprocess.check_call(cc + ["-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), str(src), "-o", exe,
                                "-L" + lib, "-lfxrx", "-Wl,-rpath," + lib])
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip() == "-1 -1"
