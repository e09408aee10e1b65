"""The header rule of the corrected reads' text (mecat_amd/csrc/cns_text.h) through libcns_poa_host.so — the function cns_text_write
runs, compiled by plain g++ — against plain Python formatting of reads_correction_can.cpp:44-46's line: every digit count from 1 to 10
in each of the four numbers, with 0, 9, 10 and 2 147 483 647 among them, and size 2.  CPU only."""
import ctypes as C
import itertools

import cns_poa_cases as P

INT_MAX = 2147483647
# one value per digit count 1 .. 10, both ends of each count, and the values the issue names
VALUES = sorted({0, 9, 10, INT_MAX, 2} | {10 ** k for k in range(10)} | {10 ** k - 1 for k in range(1, 10)} | {7, 42, 123, 4567, 89012, 345678, 9012345, 67890123, 456789012, 1234567890})
MAX_HEADER = 45


def lib():
    L = P.host_lib()
    for f in (L.cns_text_host_header_len, L.cns_text_host_header_char):
        f.restype = C.c_int
    L.cns_text_host_record_len.restype = C.c_int64
    L.cns_text_host_header_len.argtypes = L.cns_text_host_record_len.argtypes = [C.c_int32] * 4
    L.cns_text_host_header_char.argtypes = [C.c_int32] * 4 + [C.c_int]
    return L


def header_of(L, rec):
    n = L.cns_text_host_header_len(*rec)
    return n, bytes(L.cns_text_host_header_char(*rec, l) for l in range(n))


def check(L, rec):
    want = b">%d_%d_%d_%d\n" % rec
    n, got = header_of(L, rec)
    assert (n, got) == (len(want), want), rec
    assert L.cns_text_host_record_len(*rec) == len(want) + rec[3] + 1, rec
    # nothing behind the newline, nothing in front of the line
    assert all(L.cns_text_host_header_char(*rec, l) == 0 for l in (-1, n, n + 1, MAX_HEADER, 63)), rec


def test_every_digit_count_in_every_field():
    L = lib()
    assert {len(str(v)) for v in VALUES} == set(range(1, 11))
    base = (12, 345, 6789, 2)
    for field in range(4):
        for v in VALUES:
            rec = list(base)
            rec[field] = v
            check(L, tuple(rec))


def test_digit_counts_combined():
    """the fields' digit counts are independent: all combinations of a short, a middle and the longest number, and the longest header"""
    L = lib()
    for rec in itertools.product((0, 99999, INT_MAX), repeat=4):
        check(L, rec)
    n, got = header_of(L, (INT_MAX,) * 4)
    assert n == MAX_HEADER and got == b">2147483647_2147483647_2147483647_2147483647\n"


def test_size_two():
    L = lib()
    check(L, (0, 0, 2, 2))
    assert header_of(L, (0, 0, 2, 2)) == (9, b">0_0_2_2\n") and L.cns_text_host_record_len(0, 0, 2, 2) == 12
