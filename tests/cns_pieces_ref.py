"""Restatement of what mecat2cns hands to the POA for a listed window (mecat2cns/mecat_correction.cpp:62-78, meap_cns_one_indel): for
every accepted alignment of the template, in add order, CnsAln::retrieve_aln_subseqs(sb, se, qstr, tstr, sb_out)
(mecat2cns/reads_correction_aux.h:47-68) — a cursor per alignment that only moves forward.

    retrieve_literal     the cursor object and its two loops, line for line, driven over a template's listed windows in plan order
    pieces_closed_form   the numpy form the device kernels follow (mecat_amd/csrc/cns_pieces.hip): no cursor, one rule per (alignment,
                         window) pair that looks at the previous listed window only

Checker of mhip_cns_accept_templates_pieces / mhip_debug_cns_pieces (test_gpu_cns_pieces.py); the two are held against each other and
against hand-computed pieces in test_cns_pieces_ref_cpu.py.  An alignment is (qaln, saln, soff, send): two byte strings of equal length
and the m5 coordinates add_aln gets; windows are (sb, se) pairs, ascending and disjoint.  A piece is (aln, col, ncols, sb_out): the
substrings are qaln[col: col + ncols] and saln[col: col + ncols]."""
import numpy as np

PIECE_DTYPE = np.dtype([("aln", np.int32), ("col", np.int32), ("ncols", np.int32), ("sb_out", np.int32)])
GAP = ord("-")


class CnsAln:
    """reads_correction_aux.h:41-69; add_aln (:87-99) fills it"""

    def __init__(self, soff, send, qstr, tstr):
        assert len(qstr) == len(tstr)                         # :89
        self.soff = soff                                      # :91
        self.send = send                                      # :92
        self.aln_idx = 0                                      # :93
        self.aln_size = len(qstr)                             # :94
        self.qaln = bytes(qstr)                               # :95
        self.saln = bytes(tstr)                               # :97

    def retrieve_aln_subseqs(self, sb, se):
        """-> None (the reference's `false`), or (qstr, tstr, sb_out, the column the strings begin at)"""
        if se <= self.soff or sb >= self.send or self.aln_idx >= self.aln_size - 1:      # :49
            return None
        sb_out = max(self.soff, sb)                           # :50
        qstr = bytearray()                                    # :51
        tstr = bytearray()                                    # :52
        while self.soff < sb and self.aln_idx < self.aln_size - 1:                       # :53
            self.aln_idx += 1                                 # :55
            if self.saln[self.aln_idx] != GAP:                # :56
                self.soff += 1
        col = self.aln_idx
        qstr.append(self.qaln[self.aln_idx])                  # :58
        tstr.append(self.saln[self.aln_idx])                  # :59
        while self.soff < se and self.aln_idx < self.aln_size - 1:                       # :60
            self.aln_idx += 1                                 # :62
            if self.saln[self.aln_idx] != GAP:                # :63
                self.soff += 1
            qstr.append(self.qaln[self.aln_idx])              # :64
            tstr.append(self.saln[self.aln_idx])              # :65
        return bytes(qstr), bytes(tstr), sb_out, col          # :67


def as_arrays(pieces, piece_begin):
    return (np.array(pieces, dtype=PIECE_DTYPE) if pieces else np.zeros(0, PIECE_DTYPE)), np.array(piece_begin, dtype=np.int64)


def retrieve_literal(alns, windows):
    """meap_cns_one_indel's loop (:69-75) for every listed window of one template, in order -> (pieces [PIECE_DTYPE], piece_begin)"""
    cns_vec = [CnsAln(int(soff), int(send), q, s) for q, s, soff, send in alns]
    pieces, piece_begin = [], [0]
    for sb, se in windows:
        for k, a in enumerate(cns_vec):                        # :69
            r = a.retrieve_aln_subseqs(int(sb), int(se))       # :71
            if r is not None:
                qstr, tstr, sb_out, col = r
                assert qstr == a.qaln[col: col + len(qstr)] and tstr == a.saln[col: col + len(tstr)]      # a piece IS a column range
                pieces.append((k, col, len(qstr), sb_out))
        piece_begin.append(len(pieces))
    return as_arrays(pieces, piece_begin)


def column_positions(saln, soff0):
    """pos(c) = soff0 + the non-gap characters of saln[1 .. c]; pos(0) = soff0 whatever column 0 holds"""
    s = np.frombuffer(bytes(saln), dtype=np.uint8)
    step = (s != GAP).astype(np.int64)
    if len(step):
        step[0] = 0
    return int(soff0) + np.cumsum(step)


def first_column(pos, p):
    """F(p): the first column at position p, or n - 1 if there is none (pos is non-decreasing)"""
    c = int(np.searchsorted(pos, p, side="left"))
    return c if c < len(pos) and pos[c] == p else len(pos) - 1


def pieces_closed_form(alns, windows):
    """the device formulation -> (pieces, piece_begin)"""
    windows = [(int(sb), int(se)) for sb, se in windows]
    pos = [column_positions(s, soff) for q, s, soff, send in alns]
    pieces, piece_begin = [], [0]
    for w, (sb, se) in enumerate(windows):
        for k, (q, s, soff0, send) in enumerate(alns):
            n = len(s)
            if not (n >= 2 and se > soff0 and sb < send):
                continue
            if w > 0:                                          # the previous listed window took the cursor to the last column for good
                pb, pe = windows[w - 1]
                if pe > soff0 and pb < send and first_column(pos[k], pe) >= n - 1:
                    continue
            col = first_column(pos[k], max(soff0, sb))
            last = min(first_column(pos[k], se), n - 1)
            pieces.append((k, col, last - col + 1, max(int(soff0), sb)))
        piece_begin.append(len(pieces))
    return as_arrays(pieces, piece_begin)


def same_pieces(a, b):
    """None, or a short description of the first difference between two (pieces, piece_begin) pairs"""
    (pa, ba), (pb, bb) = a, b
    if not np.array_equal(ba, bb):
        w = int(np.nonzero(np.asarray(ba[: len(bb)]) != np.asarray(bb[: len(ba)]))[0][0]) if len(ba) == len(bb) else -1
        return "piece_begin differs (lengths %d / %d, first at %d)" % (len(ba), len(bb), w)
    if pa.tobytes() != pb.tobytes():
        i = int(np.nonzero(pa != pb)[0][0])
        return "piece %d (window %d): %s / %s" % (i, int(np.searchsorted(ba, i, side="right")) - 1, pa[i], pb[i])
    return None
