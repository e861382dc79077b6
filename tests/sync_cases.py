"""Traffic shared by tests/test_ref_sync.py (CPU) and tests/test_gpu_ref_sync.py: the (modulation, payload symbol count) shapes
chosen for the kernels' tile edges and tails, and how to reach them on the (modulation, length) menu.  Test infrastructure."""
import numpy as np

import ref_decode as R

BIN = 2.0 * np.pi / 512
USER_HEADER = bytes(range(101, 115))


def reach(ms, count):
    """the coded length l1 (bytes) whose symbol count is `count` for scheme ms, or None"""
    for l1 in range(0, 2200):
        if R.num_symbols(ms, l1) == count:
            return l1
    return None


def menu_counts():
    """payload symbol counts the (modulation, length) menu can reach, by ref_decode.num_symbols"""
    return {R.num_symbols(ms, l1) for ms in R.PAYLOAD_MODS for l1 in range(0, 2200)}


# (modulation, symbol count): every scheme; every reachable count in 0..10 (0 2 3 4 5 6 7 8 10: 1 and 9 are not on the menu);
# 1021..1028 as reachable, count mod 4 = 0..3; three frames above 2048
SHAPES = [(R.PSK2, 0), (R.PSK2, 8), (R.PSK2, 1024), (R.DPSK2, 8), (R.DPSK2, 2056), (R.PSK4, 1028), (R.PSK4, 4), (R.DPSK4, 8),
          (R.DPSK4, 1024), (R.ASK4, 4), (R.ASK4, 1028), (R.PSK8, 3), (R.PSK8, 1022), (R.PSK8, 1027), (R.DPSK8, 8), (R.DPSK8, 1024),
          (R.PSK16, 2), (R.PSK16, 10), (R.PSK16, 1022), (R.PSK16, 1026), (R.QAM16, 8), (R.QAM16, 1024), (R.QAM16, 2050),
          (R.QAM32, 7), (R.QAM32, 1021), (R.QAM32, 1023), (R.QAM32, 1026), (R.QAM64, 2), (R.QAM64, 7), (R.QAM64, 1023),
          (R.QAM64, 1026), (R.QAM64, 2050), (R.QAM32, 5), (R.QAM16, 6), (R.PSK8, 6)]
SMALL_COUNTS = {0, 2, 3, 4, 5, 6, 7, 8, 10}
TILE_COUNTS = {1021, 1022, 1023, 1024, 1026, 1027, 1028}
CHECKS = [R.CRC_NONE, R.CRC_8, R.CRC_16, R.CRC_24, R.CRC_32, R.CRC_CHECKSUM]


def props(ms, count, i):
    """(check, payload_len) with no FEC whose coded length gives `count` symbols"""
    l1 = reach(ms, count)
    assert l1 is not None, (ms, count)
    for k in range(len(CHECKS)):
        chk = CHECKS[(i + k) % len(CHECKS)]
        if l1 - R.crc_len(chk) >= 0:
            return chk, l1 - R.crc_len(chk)
    raise AssertionError
