"""ctypes mirror of include/mecat_hip.h (see that header for the reference functions each call replaces)."""
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))


def lib_path():
    # MECAT_HIP_LIB: a development build of the same library (e.g. the -DMECAT_DW_STATS variant, tools/dev/dw_breakdown.sh)
    return os.environ.get("MECAT_HIP_LIB") or os.path.join(_HERE, "lib", "libmecat_hip.so")


class MhipError(RuntimeError):
    pass


class Offset(C.Structure):
    _fields_ = [("offset", C.c_int32), ("size", C.c_int32)]


class Candidate(C.Structure):
    """candidate_save (mecat2pw/pw_impl.h:21-25)"""
    _fields_ = [(n, C.c_int32) for n in ("loc1", "loc2", "left1", "left2", "right1", "right2", "score", "num1", "num2",
                                         "readno", "readstart", "chain")]


class Params(C.Structure):
    _fields_ = [("maxc", C.c_int32), ("min_align_size", C.c_int32), ("min_kmer_match", C.c_int32),
                ("min_kmer_dist", C.c_int32), ("tech", C.c_int32), ("ddfs_cutoff", C.c_double)]


class AlnResult(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("ok", "query_start", "query_end", "target_start", "target_end", "matches",
                                         "columns", "blocks")]


class AlnJob(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("qid_local", "sid_local", "chain", "qstart", "sstart")]


class CnsResult(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("ok", "qoff", "qend", "soff", "send", "left_cols", "right_cols", "first_col", "last_col",
                                         "mat", "ins", "dele", "query_start", "query_end", "target_start", "target_end")]


CNS_DTYPE = np.dtype([(n, np.int32) for n, _ in CnsResult._fields_])
CAND_DTYPE = np.dtype([(n, np.int32) for n, _ in Candidate._fields_])
ALN_DTYPE = np.dtype([(n, np.int32) for n, _ in AlnResult._fields_])
JOB_DTYPE = np.dtype([(n, np.int32) for n, _ in AlnJob._fields_])
assert CAND_DTYPE.itemsize == C.sizeof(Candidate) == 48

_lib = None


class CnsOpts(C.Structure):      # mhip_cns_opts
    _fields_ = [(n, C.c_int) for n in ("tech", "input_type", "min_align_size", "min_cov", "min_size", "num_threads", "want")] + [("min_mapping_ratio", C.c_double)]


class CnsOutputs(C.Structure):      # mhip_cns_outputs
    _fields_ = [("accepted", C.c_void_p), ("count", C.c_int64), ("strings", C.c_void_p), ("strings_bytes", C.c_int64), ("jobs", C.c_int64),
                ("table", C.c_void_p), ("ident", C.c_void_p), ("table_begin", C.c_void_p),
                ("segments", C.c_void_p), ("seg_begin", C.c_void_p), ("windows", C.c_void_p), ("n_windows", C.c_int64),
                ("eranges", C.c_void_p), ("erange_begin", C.c_void_p), ("pieces", C.c_void_p), ("piece_begin", C.c_void_p),
                ("cns", C.c_void_p), ("cns_begin", C.c_void_p), ("reads", C.c_void_p), ("read_begin", C.c_void_p), ("seq", C.c_void_p),
                ("seq_bytes", C.c_int64), ("text", C.c_void_p), ("text_bytes", C.c_int64)]


def lib():
    """Loads libmecat_hip.so; raises (never falls back) when it is missing."""
    global _lib
    if _lib is not None:
        return _lib
    p = lib_path()
    if not os.path.exists(p):
        raise MhipError("%s is missing: run `make hip` (python -c 'import __graft_entry__ as g; g.build()'). "
                        "There is no CPU fallback." % p)
    L = C.CDLL(p)
    vp, i32, i64 = C.c_void_p, C.c_int, C.c_int64
    L.mhip_last_error.restype = C.c_char_p
    L.mhip_ctx_create.argtypes = [i32, vp, C.POINTER(vp)]
    L.mhip_ctx_destroy.argtypes = [vp]
    L.mhip_ctx_sync.argtypes = [vp]
    L.mhip_params_default.argtypes = [C.POINTER(Params), i32]
    L.mhip_ctx_set_profiling.argtypes = [vp, i32]
    L.mhip_ctx_kernel_stats.argtypes = [vp, C.c_char_p, C.POINTER(i64), C.POINTER(C.c_double)]
    L.mhip_ctx_kernel_names.argtypes = [vp, C.c_char_p, i32]
    L.mhip_ctx_reset_stats.argtypes = [vp]
    L.mhip_ctx_counters.argtypes = [vp, C.POINTER(i64)]
    L.mhip_debug_counter.argtypes = [vp, i32, C.POINTER(i64)]
    L.mhip_volume_upload.argtypes = [vp, vp, vp, i32, i32, i32, C.POINTER(vp)]
    L.mhip_volume_pack.argtypes = [vp, vp, i64, vp, vp, vp, i32, i32, i32, C.POINTER(vp), vp]
    L.mhip_volume_free.argtypes = [vp]
    L.mhip_volume_set_nplane.argtypes = [vp, vp, vp]
    L.mhip_volume_num_reads.argtypes = [vp]
    L.mhip_volume_num_bases.argtypes = [vp]
    L.mhip_index_build.argtypes = [vp, vp, C.POINTER(vp)]
    L.mhip_index_build_ex.argtypes = [vp, vp, i32, C.POINTER(vp)]
    L.mhip_index_free.argtypes = [vp]
    L.mhip_index_num_kmers.restype = i64
    L.mhip_index_num_kmers.argtypes = [vp]
    L.mhip_index_download.argtypes = [vp, vp, vp, vp]
    L.mhip_seed_reads.argtypes = [vp, vp, vp, vp, i32, i32, C.POINTER(Params), vp, vp]
    L.mhip_seed_reads_dev.argtypes = [vp, vp, vp, vp, i32, i32, C.POINTER(Params), vp, vp]
    L.mhip_seed_reads_strided_dev.argtypes = [vp, vp, vp, vp, i32, i32, i32, C.POINTER(Params), vp, vp]
    L.mhip_jobs_from_candidates_dev.argtypes = [vp, vp, vp, i32, i32, i32, i32, i32, i32, i32, vp, C.POINTER(i32)]
    L.mhip_align_candidates.argtypes = [vp, vp, vp, vp, i32, i32, vp]
    L.mhip_align_candidates_dev.argtypes = [vp, vp, vp, vp, i32, i32, vp]
    L.mhip_xalign_candidates.argtypes = [vp, vp, vp, vp, i32, i32, vp]
    L.mhip_xalign_candidates_dev.argtypes = [vp, vp, vp, vp, i32, i32, vp]
    L.mhip_ctx_reserve_index.argtypes = [vp, C.c_int64]
    L.mhip_ctx_buffer.argtypes = [vp, C.c_char_p, C.c_size_t, C.POINTER(vp)]
    L.mhip_download.argtypes = [vp, vp, vp, C.c_size_t]
    L.mhip_pack_candidates_dev.argtypes = [vp, vp, vp, i32, i32, vp, C.POINTER(i64)]
    L.mhip_cns_align_candidates.argtypes = [vp, vp, vp, vp, i32, C.c_double, i32, i32, vp, vp]
    L.mhip_cns_align_candidates_dev.argtypes = [vp, vp, vp, vp, i32, C.c_double, i32, i32, vp, vp]
    # multi-GPU
    L.mhip_comm_unique_id.argtypes = [vp]
    L.mhip_comm_init.argtypes = [vp, i32, i32, vp, C.POINTER(vp)]
    L.mhip_comm_init_hostfile.argtypes = [vp, i32, i32, C.c_char_p, C.c_char_p, C.POINTER(vp)]
    L.mhip_comm_destroy.argtypes = [vp]
    L.mhip_comm_barrier.argtypes = [vp]
    L.mhip_comm_info.argtypes = [vp, C.POINTER(i32), C.POINTER(i32)]
    L.mhip_comm_selftest.argtypes = [vp]
    L.mhip_comm_bytes_received.restype = i64
    L.mhip_comm_bytes_received.argtypes = [vp]
    L.mhip_shard_local_count.argtypes = [i32, i32, i32, i32, i32, i32]
    L.mhip_shard_first_read.argtypes = [i32, i32, i32, i32, i32, i32]
    L.mhip_shard_deal_rows.argtypes = [i32, vp, i32, i32, vp]
    L.mhip_seed_reads_chunked_dev.argtypes = [vp, vp, vp, vp, i32, i32, i32, i32, C.POINTER(Params), vp, vp]
    L.mhip_allgather_candidates.argtypes = [vp, vp, vp, i32, i32, i32, i32, i32, vp, vp]
    L.mhip_seed_reads_sharded.argtypes = [vp, vp, vp, vp, i32, i32, i32, i32, C.POINTER(Params), vp, vp]
    L.mhip_align_sharded.argtypes = [vp, vp, vp, i32, i32, vp, C.POINTER(i64)]
    L.mhip_sharded_tables.argtypes = [vp, C.POINTER(vp), C.POINTER(vp), C.POINTER(vp), C.POINTER(i64)]
    pvp, pi64 = C.POINTER(vp), C.POINTER(i64)
    cns_in, cns_out = [vp, vp, i32, i32, i32, C.c_double, i32], [pvp, pi64, pvp, pi64, pi64]      # the accept entry points: (cands .. threads), (accepted .. jobs)
    L.mhip_cns_accept_templates.argtypes = [vp, vp, vp] + cns_in + cns_out
    L.mhip_cns_accept_templates_ex.argtypes = [vp, vp] + cns_in + [i32] + cns_out + [pvp, pvp, pvp]
    L.mhip_debug_cns_table.argtypes = [vp, vp, i64, vp, vp, vp, i32, vp, i32, vp, vp]
    L.mhip_cns_accept_templates_plan.argtypes = [vp, vp] + cns_in + [i32, i32, i32] + cns_out + [pvp, pvp, pvp, pvp, pvp, pvp, pi64, pvp, pvp]
    L.mhip_debug_cns_plan.argtypes = [vp, vp, vp, vp, i32, vp, vp, i32, i32, i32, C.POINTER(vp), C.POINTER(vp), C.POINTER(vp), C.POINTER(i64), C.POINTER(vp),
                                      C.POINTER(vp)]
    L.mhip_debug_scan.argtypes = [vp, vp, i64, i64, vp]
    L.mhip_cns_accept_templates_pieces.argtypes = L.mhip_cns_accept_templates_plan.argtypes + [pvp, pvp]
    L.mhip_debug_cns_pieces.argtypes = [vp, vp, i64, vp, vp, vp, vp, i32, vp, i32, C.POINTER(vp), C.POINTER(vp)]
    L.mhip_cns_accept_templates_poa.argtypes = L.mhip_cns_accept_templates_pieces.argtypes + [pvp, pvp]
    L.mhip_debug_cns_poa.argtypes = [vp, vp, i64, vp, vp, vp, vp, i32, vp, i32, C.POINTER(vp), C.POINTER(vp)]
    L.mhip_cns_accept_templates_reads.argtypes = L.mhip_cns_accept_templates_poa.argtypes + [pvp, pvp, pvp, pi64]
    L.mhip_cns_format_reads.argtypes = [vp, i64, vp, i64, pvp, pi64]
    L.mhip_debug_cns_reads.argtypes = [vp, vp, vp, vp, i32, vp, vp, i64, vp, i64, vp, vp, i32, pvp, pvp, pvp, pi64]
    L.mhip_debug_cns_correct.argtypes = [vp, vp, i64, vp, vp, vp, vp, i32, vp, i32, i32, i32, i32, i32, pvp, pi64, pvp, pi64]
    L.mhip_cns_correct_templates.argtypes = [vp, vp, vp, vp, i32, C.POINTER(CnsOpts), C.POINTER(CnsOutputs)]
    L.mhip_cns_outputs_free.argtypes = [C.POINTER(CnsOutputs)]
    L.mhip_cns_outputs_free.restype = None
    L.mhip_debug_cns_text.argtypes = [vp, vp, i64, vp, i64, pvp, pi64]
    L.mhip_cns_poa_small_words.restype = i64
    L.mhip_cns_poa_small_words.argtypes = []
    L.mhip_cns_free.argtypes = [vp]
    L.mhip_host_alloc.argtypes = [C.c_size_t, C.POINTER(vp)]
    L.mhip_host_free.argtypes = [vp]
    assert L.mhip_abi_version() == 1
    _lib = L
    return L


def deal_rows(num_vols, todo, nranks):
    """rows mode's static deal (mhip_shard_deal_rows) -> (owner[num_vols], heaviest rank's cells)"""
    todo = np.ascontiguousarray(todo, dtype=np.int32)
    owner = np.zeros(max(1, num_vols), dtype=np.int32)
    mx = lib().mhip_shard_deal_rows(num_vols, todo.ctypes.data, len(todo), nranks, owner.ctypes.data)
    if mx < 0:
        raise MhipError("mhip_shard_deal_rows: bad arguments")
    return owner[:num_vols], mx


def _chk(rc):
    if rc != 0:
        raise MhipError(lib().mhip_last_error().decode())


def default_params(tech=0, **kw):
    p = Params()
    lib().mhip_params_default(C.byref(p), tech)
    for k, v in kw.items():
        setattr(p, k, v)
    return p


class Context:
    def __init__(self, device=0, stream=None):
        self.h = C.c_void_p()
        _chk(lib().mhip_ctx_create(device, stream, C.byref(self.h)))
        self.device = device

    def close(self):
        if self.h:
            lib().mhip_ctx_destroy(self.h)
            self.h = C.c_void_p()

    def sync(self):
        _chk(lib().mhip_ctx_sync(self.h))

    def set_profiling(self, on=True):
        _chk(lib().mhip_ctx_set_profiling(self.h, int(on)))

    def reset_stats(self):
        _chk(lib().mhip_ctx_reset_stats(self.h))

    def kernel_stats(self):
        buf = C.create_string_buffer(8192)
        _chk(lib().mhip_ctx_kernel_names(self.h, buf, len(buf)))
        out = {}
        for name in buf.value.decode().split("\n"):
            if not name:
                continue
            n, ms = C.c_int64(), C.c_double()
            _chk(lib().mhip_ctx_kernel_stats(self.h, name.encode(), C.byref(n), C.byref(ms)))
            out[name] = (n.value, ms.value)
        return out

    def counters(self):
        a = (C.c_int64 * 8)()
        _chk(lib().mhip_ctx_counters(self.h, a))
        names = ("lookups", "hits", "candidates", "dw_blocks", "dw_cells", "snake_bases", "aligned_bases", "aln_ok")
        return dict(zip(names, [int(x) for x in a]))

    def debug_counter(self, slot):
        """development counters 8..15 (13 / 14: strands taken by seed_strand / left to the kernel chain)"""
        v = C.c_int64()
        _chk(lib().mhip_debug_counter(self.h, slot, C.byref(v)))
        return int(v.value)


class Volume:
    """device-resident volume_t; `pac`, `offs` as load_volume() leaves them (uint8[(num_bases+3)//4], int32[n,2])"""

    def __init__(self, ctx, pac, offs, num_bases, start_read_id=0):
        pac = np.ascontiguousarray(pac, dtype=np.uint8)
        offs = np.ascontiguousarray(offs, dtype=np.int32).reshape(-1, 2)
        assert len(pac) >= (num_bases + 3) // 4
        self.h = C.c_void_p()
        self.offs = offs
        self.num_reads = len(offs)
        self.num_bases = int(num_bases)
        self.start_read_id = start_read_id
        _chk(lib().mhip_volume_upload(ctx.h, pac.ctypes.data, offs.ctypes.data, len(offs), num_bases, start_read_id,
                                      C.byref(self.h)))

    @classmethod
    def from_letters(cls, ctx, text, seq_start, line_width, offs, num_bases, start_read_id=0):
        """mhip_volume_pack: the volume packed on the device from the file's bytes -> (Volume, packed bytes uint8[(num_bases+3)//4])"""
        text = np.ascontiguousarray(np.frombuffer(text, dtype=np.uint8))
        seq_start = np.ascontiguousarray(seq_start, dtype=np.int64)
        line_width = np.ascontiguousarray(line_width, dtype=np.int32)
        offs = np.ascontiguousarray(offs, dtype=np.int32).reshape(-1, 2)
        pac = np.zeros(((num_bases + 3) // 4,), dtype=np.uint8)
        self = cls.__new__(cls)
        self.h = C.c_void_p()
        self.offs = offs
        self.num_reads = len(offs)
        self.num_bases = int(num_bases)
        self.start_read_id = start_read_id
        _chk(lib().mhip_volume_pack(ctx.h, text.ctypes.data, len(text), seq_start.ctypes.data, line_width.ctypes.data, offs.ctypes.data, len(offs),
                                    num_bases, start_read_id, C.byref(self.h), pac.ctypes.data))
        return self, pac

    @classmethod
    def from_file(cls, ctx, path):
        """reads a wrk/vol<k> file (layout of dump_volume, common/split_database.cpp:135-153)"""
        with open(path, "rb") as f:
            hdr = np.fromfile(f, dtype=np.int32, count=3)
            offs = np.fromfile(f, dtype=np.int32, count=2 * int(hdr[0])).reshape(-1, 2)
            pac = np.fromfile(f, dtype=np.uint8, count=(int(hdr[1]) + 3) // 4)
        return cls(ctx, pac, offs, int(hdr[1]), int(hdr[2]))

    def free(self):
        if self.h:
            lib().mhip_volume_free(self.h)
            self.h = C.c_void_p()


class Index:
    def __init__(self, ctx, vol, max_bucket=None):
        self.h = C.c_void_p()
        self.ctx = ctx
        if max_bucket is None:
            _chk(lib().mhip_index_build(ctx.h, vol.h, C.byref(self.h)))
        else:
            _chk(lib().mhip_index_build_ex(ctx.h, vol.h, int(max_bucket), C.byref(self.h)))

    @property
    def num_kmers(self):
        return lib().mhip_index_num_kmers(self.h)

    def download(self, want_counts=True, want_offsets=True):
        counts = np.empty(1 << 26, dtype=np.int32) if want_counts else None
        offs = np.empty(self.num_kmers, dtype=np.int32) if want_offsets else None
        _chk(lib().mhip_index_download(self.ctx.h, self.h, counts.ctypes.data if want_counts else None,
                                       offs.ctypes.data if want_offsets else None))
        return counts, offs

    def download_aux(self):
        """(slots uint16[num_kmers], recs uint32[4^13, 4] or None, cut_step): the side arrays of the seeding stage (test hook)"""
        slots = np.empty(self.num_kmers, dtype=np.uint16)
        recs = np.empty((1 << 26, 4), dtype=np.uint32)
        cs = C.c_int()
        lib().mhip_index_download_aux.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_int)]
        rc = lib().mhip_index_download_aux(self.ctx.h, self.h, slots.ctypes.data, recs.ctypes.data, C.byref(cs))
        if rc < 0:
            raise MhipError(lib().mhip_last_error().decode())
        return slots, (recs if rc == 0 else None), cs.value

    def free(self):
        if self.h:
            lib().mhip_index_free(self.h)
            self.h = C.c_void_p()


ASM_CAND_DTYPE = np.dtype([(n, np.int32) for n in ("loc1", "loc2", "left1", "left2", "right1", "right2", "score", "num1", "num2", "readno",
                                                    "readstart", "chain")])


def asm_seed_reads(ctx, idx, block, reads, rid_begin, rid_end):
    """mhip_asm_seed_reads: the candidate stage of mecat2asmpw's pairwise_mapping -> (cands [n, 100] ASM_CAND_DTYPE, counts int32[n])"""
    n = rid_end - rid_begin
    out = np.zeros((n, 100), dtype=ASM_CAND_DTYPE)
    cnt = np.zeros(n, dtype=np.int32)
    lib().mhip_asm_seed_reads.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p]
    _chk(lib().mhip_asm_seed_reads(ctx.h, idx.h, block.h, reads.h, rid_begin, rid_end, out.ctypes.data, cnt.ctypes.data))
    return out, cnt


ASM_JOB_DTYPE = np.dtype([(n, np.int32) for n in ("xid", "yid", "chain", "lx", "ly", "lnx", "lny", "rx", "ry", "rnx", "rny", "pad")])
assert ASM_JOB_DTYPE.itemsize == 48


def volume_set_nplane(ctx, vol, nplane):
    """mhip_volume_set_nplane: the second 2-bit plane of a volume (non-zero at every base that is not A, C, G, T); None removes it"""
    if nplane is not None:
        nplane = np.ascontiguousarray(nplane, dtype=np.uint8)
        assert len(nplane) >= (vol.num_bases + 3) // 4
    _chk(lib().mhip_volume_set_nplane(ctx.h, vol.h, nplane.ctypes.data if nplane is not None else None))


class RefCandidate(C.Structure):
    """mhip_ref_candidate (candidate_save, mecat2ref/mecat2ref_defs.h:88-93)"""
    _fields_ = [(n, C.c_int64) for n in ("loc1", "loc2", "left1", "left2", "right1", "right2")] + [(n, C.c_int32) for n in ("score", "num1", "num2", "chain")]


class RefSeedParams(C.Structure):      # mhip_ref_seed_params
    _fields_ = [("maxc", C.c_int32), ("round", C.c_int32), ("ddfs_cutoff", C.c_double)]


REF_CAND_DTYPE = np.dtype([(n, np.int64 if t is C.c_int64 else np.int32) for n, t in RefCandidate._fields_])
assert REF_CAND_DTYPE.itemsize == C.sizeof(RefCandidate) == 64 and C.sizeof(RefSeedParams) == 16


def ref_seed_params(tech=0, **kw):
    """mhip_ref_seed_params_default, then the given members"""
    p = RefSeedParams()
    lib().mhip_ref_seed_params_default.argtypes = [C.POINTER(RefSeedParams), C.c_int]
    lib().mhip_ref_seed_params_default.restype = None
    lib().mhip_ref_seed_params_default(C.byref(p), tech)
    for k, v in kw.items():
        setattr(p, k, v)
    return p


_REF_SEED_ARGS = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.POINTER(RefSeedParams), C.c_void_p, C.c_void_p]


def ref_seed_reads(ctx, idx, ref, reads, rid_begin, rid_end, params):
    """mhip_ref_seed_reads: mecat2ref's seeding and candidate selection -> (cands [n, maxc] REF_CAND_DTYPE, counts int32[n])"""
    n = max(rid_end - rid_begin, 0)
    out = np.zeros((n, max(params.maxc, 1)), dtype=REF_CAND_DTYPE)
    cnt = np.zeros(n, dtype=np.int32)
    lib().mhip_ref_seed_reads.argtypes = _REF_SEED_ARGS
    _chk(lib().mhip_ref_seed_reads(ctx.h, idx.h, ref.h, reads.h, rid_begin, rid_end, C.byref(params), out.ctypes.data, cnt.ctypes.data))
    return out, cnt


def ref_seed_reads_dev(ctx, idx, ref, reads, rid_begin, rid_end, params, d_out, d_counts):
    """mhip_ref_seed_reads_dev: the same into device buffers (e.g. of mhip_ctx_buffer)"""
    lib().mhip_ref_seed_reads_dev.argtypes = _REF_SEED_ARGS
    _chk(lib().mhip_ref_seed_reads_dev(ctx.h, idx.h, ref.h, reads.h, rid_begin, rid_end, C.byref(params), d_out, d_counts))


def ref_seed_stats():
    """mhip_ref_seed_stats of the last call: dict(reads, redone, waves, pool)"""
    v = (C.c_int64 * 4)()
    lib().mhip_ref_seed_stats.restype = None
    lib().mhip_ref_seed_stats(v)
    return dict(reads=int(v[0]), redone=int(v[1]), waves=int(v[2]), pool=int(v[3]))


class RefResult(C.Structure):
    """mhip_ref_result: a TempResult (mecat2ref/output.h) without its strings"""
    _fields_ = [(n, C.c_int32) for n in ("ok", "chain", "vscore", "qb", "qe", "qs")] + [("sb", C.c_int64), ("se", C.c_int64), ("cols", C.c_int32), ("pad", C.c_int32)]


REF_RESULT_DTYPE = np.dtype([(n, np.int64 if t is C.c_int64 else np.int32) for n, t in RefResult._fields_])
assert REF_RESULT_DTYPE.itemsize == C.sizeof(RefResult) == 48

_REF_EXT_ARGS = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.POINTER(C.c_int64)]


def ref_extend_run(ctx, ref, reads, rid_begin, rid_end, maxc, cands, counts, tech=0):
    """mhip_ref_extend_run: mecat2ref's extension of the listed candidates (host lists, ref_seed_reads' layout) -> total words"""
    cands = np.ascontiguousarray(cands, dtype=REF_CAND_DTYPE)
    counts = np.ascontiguousarray(counts, dtype=np.int32)
    assert cands.size == max(rid_end - rid_begin, 0) * maxc and len(counts) == max(rid_end - rid_begin, 0)
    tot = C.c_int64()
    lib().mhip_ref_extend_run.argtypes = _REF_EXT_ARGS
    _chk(lib().mhip_ref_extend_run(ctx.h, ref.h, reads.h, rid_begin, rid_end, maxc, tech, cands.ctypes.data, counts.ctypes.data, C.byref(tot)))
    return tot.value


def ref_extend_run_dev(ctx, ref, reads, rid_begin, rid_end, maxc, d_cands, d_counts, tech=0):
    """mhip_ref_extend_run_dev: the same on device lists (mhip_ref_seed_reads_dev's output) -> total words"""
    tot = C.c_int64()
    lib().mhip_ref_extend_run_dev.argtypes = _REF_EXT_ARGS
    _chk(lib().mhip_ref_extend_run_dev(ctx.h, ref.h, reads.h, rid_begin, rid_end, maxc, tech, d_cands, d_counts, C.byref(tot)))
    return tot.value


def ref_extend_fetch(ctx, n, maxc, total_words):
    """mhip_ref_extend_fetch -> (res [n, maxc] REF_RESULT_DTYPE, word_offs uint64[n * maxc + 1], words uint32[total_words])"""
    res = np.zeros((n, maxc), dtype=REF_RESULT_DTYPE)
    offs = np.zeros(n * maxc + 1, dtype=np.uint64)
    words = np.zeros(max(total_words, 1), dtype=np.uint32)
    lib().mhip_ref_extend_fetch.argtypes = [C.c_void_p] * 4
    _chk(lib().mhip_ref_extend_fetch(ctx.h, res.ctypes.data, offs.ctypes.data, words.ctypes.data))
    return res, offs, words[:total_words]


def ref_extend(ctx, ref, reads, rid_begin, rid_end, maxc, cands, counts, tech=0):
    """run + fetch -> (res, word_offs, words)"""
    tot = ref_extend_run(ctx, ref, reads, rid_begin, rid_end, maxc, cands, counts, tech)
    return ref_extend_fetch(ctx, max(rid_end - rid_begin, 0), maxc, tot)


_REF_XEXT_ARGS = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.POINTER(C.c_int64)]


def ref_xextend_run(ctx, ref, reads, rid_begin, rid_end, maxc, cands, counts):
    """mhip_ref_xextend_run: the extension in nanopore mode (XdropAligner) of host lists -> total words; ref_extend_fetch fetches"""
    cands = np.ascontiguousarray(cands, dtype=REF_CAND_DTYPE)
    counts = np.ascontiguousarray(counts, dtype=np.int32)
    assert cands.size == max(rid_end - rid_begin, 0) * maxc and len(counts) == max(rid_end - rid_begin, 0)
    tot = C.c_int64()
    lib().mhip_ref_xextend_run.argtypes = _REF_XEXT_ARGS
    _chk(lib().mhip_ref_xextend_run(ctx.h, ref.h, reads.h, rid_begin, rid_end, maxc, cands.ctypes.data, counts.ctypes.data, C.byref(tot)))
    return tot.value


def ref_xextend_run_dev(ctx, ref, reads, rid_begin, rid_end, maxc, d_cands, d_counts):
    """mhip_ref_xextend_run_dev: the same on device lists (mhip_ref_seed_reads_dev's output) -> total words"""
    tot = C.c_int64()
    lib().mhip_ref_xextend_run_dev.argtypes = _REF_XEXT_ARGS
    _chk(lib().mhip_ref_xextend_run_dev(ctx.h, ref.h, reads.h, rid_begin, rid_end, maxc, d_cands, d_counts, C.byref(tot)))
    return tot.value


def ref_xextend(ctx, ref, reads, rid_begin, rid_end, maxc, cands, counts):
    """run + fetch -> (res, word_offs, words)"""
    tot = ref_xextend_run(ctx, ref, reads, rid_begin, rid_end, maxc, cands, counts)
    return ref_extend_fetch(ctx, max(rid_end - rid_begin, 0), maxc, tot)


def ref_xextend_stats():
    """mhip_ref_xextend_stats of the last run: dict(slots, slices, redone (blocks redone with the wide block), store_words)"""
    v = (C.c_int64 * 4)()
    lib().mhip_ref_xextend_stats.restype = None
    lib().mhip_ref_xextend_stats(v)
    return dict(slots=int(v[0]), slices=int(v[1]), redone=int(v[2]), store_words=int(v[3]))


def ref_extend_stats():
    """mhip_ref_extend_stats of the last run: dict(slots, slices, row_bytes, store_words)"""
    v = (C.c_int64 * 4)()
    lib().mhip_ref_extend_stats.restype = None
    lib().mhip_ref_extend_stats(v)
    return dict(slots=int(v[0]), slices=int(v[1]), row_bytes=int(v[2]), store_words=int(v[3]))


class RefRescueParams(C.Structure):      # mhip_ref_rescue_params
    _fields_ = [("maxc", C.c_int32), ("round", C.c_int32), ("num_output", C.c_int32), ("tech", C.c_int32), ("ddfs_cutoff", C.c_double)]


# mhip_ref_rescue_state: what rescue_clipped_align holds when it starts to look for rescue candidates (mecat2ref_aux.cpp:328-341)
REF_RESCUE_STATE_DTYPE = np.dtype([("naln", np.int32), ("go_on", np.int32), ("nres", np.int32), ("qs", np.int32), ("slot", np.int8, 16), ("id", np.int8, 16)])
REF_RESCUE_TRIES = 6
assert REF_RESCUE_STATE_DTYPE.itemsize == 48 and C.sizeof(RefRescueParams) == 24


def ref_rescue_params(tech=0, **kw):
    """mhip_ref_rescue_params_default, then the given members"""
    p = RefRescueParams()
    lib().mhip_ref_rescue_params_default.argtypes = [C.POINTER(RefRescueParams), C.c_int]
    lib().mhip_ref_rescue_params_default.restype = None
    lib().mhip_ref_rescue_params_default(C.byref(p), tech)
    for k, v in kw.items():
        setattr(p, k, v)
    return p


_REF_RESCUE_ARGS = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.POINTER(RefRescueParams), C.c_void_p, C.POINTER(C.c_int64)]


def ref_rescue_run(ctx, idx, ref, reads, rid_begin, rid_end, params, res):
    """mhip_ref_rescue_run: mecat2ref's rescue and result order on host results res [n, maxc] (ref_extend_fetch's) -> total words of
    the rescue results"""
    res = np.ascontiguousarray(res, dtype=REF_RESULT_DTYPE)
    assert res.shape == (max(rid_end - rid_begin, 0), params.maxc)
    tot = C.c_int64()
    lib().mhip_ref_rescue_run.argtypes = _REF_RESCUE_ARGS
    _chk(lib().mhip_ref_rescue_run(ctx.h, idx.h, ref.h, reads.h, rid_begin, rid_end, C.byref(params), res.ctypes.data, C.byref(tot)))
    return tot.value


def ref_rescue_run_dev(ctx, idx, ref, reads, rid_begin, rid_end, params, d_res=None):
    """mhip_ref_rescue_run_dev: the same on device results; None = those of the last ref_extend_run* on this context"""
    tot = C.c_int64()
    lib().mhip_ref_rescue_run_dev.argtypes = _REF_RESCUE_ARGS
    _chk(lib().mhip_ref_rescue_run_dev(ctx.h, idx.h, ref.h, reads.h, rid_begin, rid_end, C.byref(params), d_res, C.byref(tot)))
    return tot.value


def ref_xrescue_run(ctx, idx, ref, reads, rid_begin, rid_end, params, res):
    """mhip_ref_xrescue_run: the rescue stage in nanopore mode (params.tech must be 1) on host results -> total words; ref_rescue_fetch
    fetches"""
    res = np.ascontiguousarray(res, dtype=REF_RESULT_DTYPE)
    assert res.shape == (max(rid_end - rid_begin, 0), params.maxc)
    tot = C.c_int64()
    lib().mhip_ref_xrescue_run.argtypes = _REF_RESCUE_ARGS
    _chk(lib().mhip_ref_xrescue_run(ctx.h, idx.h, ref.h, reads.h, rid_begin, rid_end, C.byref(params), res.ctypes.data, C.byref(tot)))
    return tot.value


def ref_xrescue_run_dev(ctx, idx, ref, reads, rid_begin, rid_end, params, d_res=None):
    """mhip_ref_xrescue_run_dev: the same on device results; None = those of the last ref_xextend_run* on this context"""
    tot = C.c_int64()
    lib().mhip_ref_xrescue_run_dev.argtypes = _REF_RESCUE_ARGS
    _chk(lib().mhip_ref_xrescue_run_dev(ctx.h, idx.h, ref.h, reads.h, rid_begin, rid_end, C.byref(params), d_res, C.byref(tot)))
    return tot.value


def ref_rescue_fetch(ctx, n, num_output, total_words):
    """mhip_ref_rescue_fetch -> dict(out_slots int32[n, 3 * num_output], out_counts, cands [n, 6] REF_CAND_DTYPE, counts, res [n, 6]
    REF_RESULT_DTYPE, word_offs uint64[6 n + 1], words); candidates and results behind a read's count are zeroed"""
    T = REF_RESCUE_TRIES
    slots = np.full((n, 3 * num_output), -1, dtype=np.int32)
    oc, cnt = np.zeros(n, dtype=np.int32), np.zeros(n, dtype=np.int32)
    cands = np.zeros((n, T), dtype=REF_CAND_DTYPE)
    res = np.zeros((n, T), dtype=REF_RESULT_DTYPE)
    offs = np.zeros(n * T + 1, dtype=np.uint64)
    words = np.zeros(max(total_words, 1), dtype=np.uint32)
    lib().mhip_ref_rescue_fetch.argtypes = [C.c_void_p] * 8
    _chk(lib().mhip_ref_rescue_fetch(ctx.h, slots.ctypes.data, oc.ctypes.data, cands.ctypes.data, cnt.ctypes.data, res.ctypes.data, offs.ctypes.data, words.ctypes.data))
    behind = np.arange(T)[None, :] >= cnt[:, None]
    cands[behind] = np.zeros((), dtype=REF_CAND_DTYPE)
    return dict(out_slots=slots, out_counts=oc, cands=cands, counts=cnt, res=res, word_offs=offs, words=words[:total_words])


def ref_rescue_stats():
    """mhip_ref_rescue_stats of the last run: dict(reads, went_on, candidates, redone)"""
    v = (C.c_int64 * 4)()
    lib().mhip_ref_rescue_stats.restype = None
    lib().mhip_ref_rescue_stats(v)
    return dict(reads=int(v[0]), went_on=int(v[1]), candidates=int(v[2]), redone=int(v[3]))


def debug_ref_rescue_prep(ctx, params, res):
    """test hook: ref_rescue_prep (the sort, the containment filter and the full-alignment test of rescue_clipped_align) on host
    results res [n, maxc] REF_RESULT_DTYPE -> states [n] REF_RESCUE_STATE_DTYPE"""
    res = np.ascontiguousarray(res, dtype=REF_RESULT_DTYPE)
    assert res.ndim == 2 and res.shape[1] == params.maxc
    st = np.zeros(len(res), dtype=REF_RESCUE_STATE_DTYPE)
    lib().mhip_debug_ref_rescue_prep.argtypes = [C.c_void_p, C.POINTER(RefRescueParams), C.c_int, C.c_void_p, C.c_void_p]
    _chk(lib().mhip_debug_ref_rescue_prep(ctx.h, C.byref(params), len(res), res.ctypes.data, st.ctypes.data))
    return st


def debug_ref_rescue_finish(ctx, params, res, states, rescue_counts, rescue_meta, rescue_res):
    """test hook: ref_rescue_finish (the attach tests, the second sort with its cut and output_results) on hand-made states and rescue
    results.  rescue_meta int32[n, 6] = owner entry | side << 8, rescue_res [n, 6] REF_RESULT_DTYPE
    -> (out_slots int32[n, 3 * num_output], out_counts int32[n])"""
    res = np.ascontiguousarray(res, dtype=REF_RESULT_DTYPE)
    st = np.ascontiguousarray(states, dtype=REF_RESCUE_STATE_DTYPE)
    cnt = np.ascontiguousarray(rescue_counts, dtype=np.int32)
    meta = np.ascontiguousarray(rescue_meta, dtype=np.int32)
    rres = np.ascontiguousarray(rescue_res, dtype=REF_RESULT_DTYPE)
    n = len(st)
    assert res.shape == (n, params.maxc) and cnt.shape == (n,) and meta.shape == (n, REF_RESCUE_TRIES) and rres.shape == (n, REF_RESCUE_TRIES)
    slots = np.zeros((n, 3 * max(params.num_output, 1)), dtype=np.int32)
    oc = np.zeros(n, dtype=np.int32)
    lib().mhip_debug_ref_rescue_finish.argtypes = [C.c_void_p, C.POINTER(RefRescueParams), C.c_int] + [C.c_void_p] * 7
    _chk(lib().mhip_debug_ref_rescue_finish(ctx.h, C.byref(params), n, res.ctypes.data, st.ctypes.data, cnt.ctypes.data, meta.ctypes.data, rres.ctypes.data,
                                            slots.ctypes.data, oc.ctypes.data))
    return slots, oc


def asm_jobs_from_candidates(cands, counts, rid_begin=0):
    """the (candidate, both directions) jobs of an asm_seed_reads table, read by read in list order (include/mecat_hip.h: x0 = loc1 - 1 -
    readstart; left from (x0 + 12, loc2 + 12) with left1 / left2 bases, right from (x0, loc2) with right1 / right2) -> [n] ASM_JOB_DTYPE"""
    counts = np.asarray(counts)
    mask = np.arange(cands.shape[1])[None, :] < counts[:, None]
    c = cands[mask]
    jobs = np.zeros(len(c), dtype=ASM_JOB_DTYPE)
    x0 = c["loc1"] - 1 - c["readstart"]
    jobs["xid"], jobs["chain"] = c["readno"], c["chain"]
    jobs["yid"] = rid_begin + np.repeat(np.arange(len(counts), dtype=np.int32), counts)
    jobs["lx"], jobs["ly"], jobs["lnx"], jobs["lny"] = x0 + 12, c["loc2"] + 12, c["left1"], c["left2"]
    jobs["rx"], jobs["ry"], jobs["rnx"], jobs["rny"] = x0, c["loc2"], c["right1"], c["right2"]
    return jobs


def asm_extend(ctx, block, reads, jobs, dir_cols_cap):
    """mhip_asm_extend: the extension loop of mecat2asmpw / mecat2trimpw, fixed-stride form
    -> (dirs int32[2 n, 6] = {cols, x bases, y bases, y-only, x-only, 0}, ops uint32[2 n, dir_cols_cap // 16])"""
    jobs = np.ascontiguousarray(jobs, dtype=ASM_JOB_DTYPE)
    n = len(jobs)
    dirs = np.zeros((2 * n, 6), dtype=np.int32)
    ops = np.zeros((2 * n, max(dir_cols_cap, 0) // 16), dtype=np.uint32)
    L = lib()
    L.mhip_asm_extend.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p]
    _chk(L.mhip_asm_extend(ctx.h, block.h, reads.h, jobs.ctypes.data, n, dir_cols_cap, dirs.ctypes.data, ops.ctypes.data))
    return dirs, ops


def asm_extend_run(ctx, block, reads, jobs, dir_cols_cap):
    """mhip_asm_extend_run: extends the batch, leaves the results on the device -> the 32-bit words of all directions' columns"""
    jobs = np.ascontiguousarray(jobs, dtype=ASM_JOB_DTYPE)
    total = C.c_int64()
    L = lib()
    L.mhip_asm_extend_run.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.POINTER(C.c_int64)]
    _chk(L.mhip_asm_extend_run(ctx.h, block.h, reads.h, jobs.ctypes.data, len(jobs), dir_cols_cap, C.byref(total)))
    return int(total.value)


def asm_extend_fetch(ctx, n, total_words):
    """mhip_asm_extend_fetch for the last asm_extend_run on the context (n = its jobs, total_words = what it returned)
    -> (dirs int32[2 n, 6], word_offs uint64[2 n + 1], ops_dense uint32[total_words])"""
    dirs = np.zeros((2 * n, 6), dtype=np.int32)
    offs = np.zeros(2 * n + 1, dtype=np.uint64)
    dense = np.zeros(max(total_words, 1), dtype=np.uint32)
    L = lib()
    L.mhip_asm_extend_fetch.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
    _chk(L.mhip_asm_extend_fetch(ctx.h, n, dirs.ctypes.data, offs.ctypes.data, dense.ctypes.data))
    return dirs, offs, dense[:total_words]


def seed_reads(ctx, idx, ref, reads, rid_begin, rid_end, params):
    """-> (cands structured array [n, maxc], counts int32[n]) on the host"""
    n = rid_end - rid_begin
    out = np.zeros((n, params.maxc), dtype=CAND_DTYPE)
    cnt = np.zeros(n, dtype=np.int32)
    _chk(lib().mhip_seed_reads(ctx.h, idx.h, ref.h, reads.h, rid_begin, rid_end, C.byref(params), out.ctypes.data,
                               cnt.ctypes.data))
    return out, cnt


def seed_reads_dev(ctx, idx, ref, reads, rid_begin, rid_end, params, d_out, d_counts):
    _chk(lib().mhip_seed_reads_dev(ctx.h, idx.h, ref.h, reads.h, rid_begin, rid_end, C.byref(params), d_out, d_counts))


def seed_reads_strided_dev(ctx, idx, ref, reads, rid_begin, rid_stride, n, params, d_out, d_counts):
    _chk(lib().mhip_seed_reads_strided_dev(ctx.h, idx.h, ref.h, reads.h, rid_begin, rid_stride, n, C.byref(params), d_out, d_counts))


def jobs_from_candidates_dev(ctx, d_cands, d_counts, n_reads, maxc, rid_begin, rid_stride, ref_start_id, part_index, part_count,
                             d_jobs):
    n = C.c_int32(0)
    _chk(lib().mhip_jobs_from_candidates_dev(ctx.h, d_cands, d_counts, n_reads, maxc, rid_begin, rid_stride, ref_start_id,
                                             part_index, part_count, d_jobs, C.byref(n)))
    return n.value


def align_candidates(ctx, ref, reads, jobs, min_align_size, tech=0):
    """tech 0: dw / DiffAligner, tech 1: X-drop aligner (nanopore mode)"""
    jobs = np.ascontiguousarray(jobs, dtype=JOB_DTYPE)
    out = np.zeros(len(jobs), dtype=ALN_DTYPE)
    if len(jobs):
        fn = lib().mhip_xalign_candidates if tech == 1 else lib().mhip_align_candidates
        _chk(fn(ctx.h, ref.h, reads.h, jobs.ctypes.data, len(jobs), min_align_size, out.ctypes.data))
    return out


def align_candidates_dev(ctx, ref, reads, d_jobs, n, min_align_size, d_out):
    _chk(lib().mhip_align_candidates_dev(ctx.h, ref.h, reads.h, d_jobs, n, min_align_size, d_out))


def cns_align_candidates(ctx, ref, reads, jobs, error_rate, min_align_size, dir_cols_cap):
    """mecat2cns re-aligner (GetAlignment).  -> (results [n] CNS_DTYPE, ops [n, 2, dir_cols_cap / 16] uint32)"""
    jobs = np.ascontiguousarray(jobs, dtype=JOB_DTYPE)
    n = len(jobs)
    res = np.zeros(n, dtype=CNS_DTYPE)
    ops = np.zeros((n, 2, dir_cols_cap // 16), dtype=np.uint32)
    if n:
        _chk(lib().mhip_cns_align_candidates(ctx.h, ref.h, reads.h, jobs.ctypes.data, n, float(error_rate), min_align_size, dir_cols_cap,
                                             res.ctypes.data, ops.ctypes.data))
    return res, ops


def cns_expand(res, ops_row, qcodes, tcodes):
    """Rebuild the aligned strings of one result from its ops (the host side of the 2-bit column format): qcodes = the
    query read as the aligner saw it (reverse-complemented when chain != 0), tcodes = the template.  -> (qaln, saln) over
    "ACGT-", i.e. m5qaln / m5saln."""
    def unpack(words, ncols):
        w = np.asarray(words[: (ncols + 15) // 16], dtype=np.uint32)
        cols = ((w[:, None] >> (2 * np.arange(16, dtype=np.uint32))[None, :]) & 3).reshape(-1)
        return cols[:ncols].astype(np.uint8)
    left = unpack(ops_row[0], int(res["left_cols"]))[::-1]
    right = unpack(ops_row[1], int(res["right_cols"]))
    ops = np.concatenate([left, right])
    dec = np.frombuffer(b"ACGT", dtype=np.uint8)
    qi = int(res["query_start"]) + np.cumsum(ops != 1) - (ops != 1)
    ti = int(res["target_start"]) + np.cumsum(ops != 2) - (ops != 2)
    qs = np.where(ops == 1, ord("-"), dec[np.asarray(qcodes)[np.minimum(qi, len(qcodes) - 1)]]).astype(np.uint8)
    ts = np.where(ops == 2, ord("-"), dec[np.asarray(tcodes)[np.minimum(ti, len(tcodes) - 1)]]).astype(np.uint8)
    a, b = int(res["first_col"]), int(res["last_col"])
    return qs[a:b].tobytes(), ts[a:b].tobytes()


EXT_CAND_DTYPE = np.dtype([(n, np.int32) for n in ("qdir", "qid", "qext", "qsize", "qoff", "qend", "sdir", "sid", "sext", "ssize", "soff", "send",
                                                     "score")])
ACCEPTED_DTYPE = np.dtype([("template_index", np.int32), ("qid", np.int32), ("sid", np.int32), ("qoff", np.int32), ("qend", np.int32),
                           ("soff", np.int32), ("send", np.int32), ("aln_size", np.int32), ("cand_index", np.int64), ("str_offset", np.int64)])
assert EXT_CAND_DTYPE.itemsize == 52 and ACCEPTED_DTYPE.itemsize == 48


def cns_accept_templates(ctx, vol, host_pac, cands, tmpl_begin, tech, min_align_size, min_mapping_ratio, threads=8):
    """mecat2cns' accept loop for a batch of templates.  cands: [n] EXT_CAND_DTYPE (or [n, 13] int32) grouped by template, sorted in
    place.  -> (accepted [k] ACCEPTED_DTYPE, strings as a uint8 array over the library's buffer, number of alignments computed)"""
    # (host_pac is no longer read by the library: the strings are built on the device; kept in the signature)
    return _cns_accept("", ctx, vol, cands, tmpl_begin, tech, min_align_size, min_mapping_ratio, CNS_WANT_STRINGS, threads=threads)[:3]


CNS_WANT_STRINGS, CNS_WANT_TABLE = 1, 2
TABLE_DTYPE = np.dtype([("base", np.uint8), ("mat_cnt", np.uint8), ("ins_cnt", np.uint8), ("del_cnt", np.uint8)])      # CnsTableItem
IDENT_FMAT, IDENT_FDEL, IDENT_FINS, IDENT_UNDS = 1, 2, 4, 8


def _cns_buffer(ptr, nbytes):
    """uint8 array over a buffer of the library (no copy), released with mhip_cns_free when the array goes"""
    import weakref
    if not ptr.value or not nbytes:
        lib().mhip_cns_free(ptr)
        return np.zeros(0, np.uint8)
    a = np.ctypeslib.as_array(C.cast(ptr, C.POINTER(C.c_uint8)), shape=(nbytes,))
    weakref.finalize(a, lib().mhip_cns_free, C.c_void_p(ptr.value))
    return a


def cns_accept_templates_ex(ctx, vol, cands, tmpl_begin, tech, min_align_size, min_mapping_ratio, want, threads=8):
    """cns_accept_templates with the outputs chosen by `want` (CNS_WANT_STRINGS | CNS_WANT_TABLE): the consensus tables of the templates
    (meap_add_one_aln) and their ident bytes (identify_one_consensus_item) come from the device.
    -> (accepted, strings, number of alignments computed, table [TABLE_DTYPE], ident [uint8], table_begin [templates + 1]): template t
    owns table[table_begin[t]: table_begin[t + 1]], one item per base of the read.  Without CNS_WANT_STRINGS `strings` is empty and every
    str_offset -1; without CNS_WANT_TABLE the last three are empty."""
    return _cns_accept("_ex", ctx, vol, cands, tmpl_begin, tech, min_align_size, min_mapping_ratio, want, threads=threads)[:6]


def debug_cns_table(ctx, buf, off, lens, soff, tmpl_letters):
    """test hook: the accept stage's table kernels over pairs of aligned strings to one template.  buf: uint8 buffer, pair p = q at
    off[p] (lens[p] characters + NUL), s right behind it; soff[p] = template position of its first template base; tmpl_letters: bytes.
    -> (table [len(tmpl_letters)] TABLE_DTYPE, ident uint8)"""
    buf = np.ascontiguousarray(buf, dtype=np.uint8)
    off = np.ascontiguousarray(off, dtype=np.int64)
    lens = np.ascontiguousarray(lens, dtype=np.int32)
    soff = np.ascontiguousarray(soff, dtype=np.int32)
    let = np.frombuffer(bytes(tmpl_letters), dtype=np.uint8)
    assert len(off) == len(lens) == len(soff)
    table = np.zeros(len(let), TABLE_DTYPE)
    ident = np.zeros(len(let), np.uint8)
    _chk(lib().mhip_debug_cns_table(ctx.h, buf.ctypes.data, len(buf), off.ctypes.data, lens.ctypes.data, soff.ctypes.data, len(off), let.ctypes.data, len(let),
                                    table.ctypes.data, ident.ctypes.data))
    return table, ident


CNS_WANT_PLAN = 4
SEGMENT_DTYPE = np.dtype([("template_index", np.int32), ("beg", np.int32), ("end", np.int32), ("n_anchors", np.int32), ("win_begin", np.int64),
                          ("win_end", np.int64)])                                                                    # mhip_cns_segment
WINDOW_DTYPE = np.dtype([("sb", np.int32), ("se", np.int32), ("cov", np.int32), ("segment", np.int32)])              # mhip_cns_window
assert SEGMENT_DTYPE.itemsize == 32 and WINDOW_DTYPE.itemsize == 16


def _cns_take(ptr, dtype, n):
    """a copy of n records behind a pointer of the library (NULL: none), which is released"""
    if ptr.value and n:
        a = np.ctypeslib.as_array(C.cast(ptr, C.POINTER(C.c_uint8)), shape=(n * np.dtype(dtype).itemsize,)).view(dtype).copy()
    else:
        a = np.zeros(0, dtype)
    lib().mhip_cns_free(ptr)
    return a


def _cns_plan_out(seg, segb, win, nwin, er, erb, ntmpl):
    """the six plan outputs -> dict(segments, seg_begin, windows, eranges [k, 2], erange_begin).  Segments and windows are arrays over the
    library's buffers (gigabytes of windows at config 2: no copy), released when they go; the small ones are copied and released"""
    seg_begin = _cns_take(segb, np.int64, ntmpl + 1)
    erange_begin = _cns_take(erb, np.int64, ntmpl + 1)
    nseg = int(seg_begin[-1]) if len(seg_begin) else 0
    ner = int(erange_begin[-1]) if len(erange_begin) else 0
    return dict(segments=_cns_buffer(seg, nseg * SEGMENT_DTYPE.itemsize).view(SEGMENT_DTYPE), seg_begin=seg_begin,
                windows=_cns_buffer(win, int(nwin.value) * WINDOW_DTYPE.itemsize).view(WINDOW_DTYPE),
                eranges=_cns_take(er, np.int32, 2 * ner).reshape(-1, 2), erange_begin=erange_begin)


def _cns_accept(entry, ctx, vol, cands, tmpl_begin, tech, min_align_size, min_mapping_ratio, want, min_cov=None, min_size=None, threads=8):
    """the body of the six cns_accept_templates* bindings: mhip_cns_accept_templates + entry ("", "_ex", "_plan", "_pieces", "_poa", "_reads"),
    which decides the out-parameters behind out_jobs.  -> (accepted, strings, jobs, table, ident, table_begin, plan dict or None), and
    for "_reads" the reads dict or None behind it"""
    cands = np.ascontiguousarray(cands)
    tb = np.ascontiguousarray(tmpl_begin, dtype=np.int64)
    want = int(want)
    acc, st, tab, idn, tbeg, seg, segb, win, er, erb, pc, pcb, cn, cnb = (C.c_void_p() for _ in range(14))
    na, sb, nj, nwin = (C.c_int64() for _ in range(4))
    rd, rdb, sq = (C.c_void_p() for _ in range(3))
    sqb = C.c_int64()
    outs = [acc, na, st, sb, nj] + [tab, idn, tbeg, seg, segb, win, nwin, er, erb, pc, pcb, cn, cnb, rd, rdb, sq, sqb][: {"": 0, "_ex": 3, "_plan": 9, "_pieces": 11, "_poa": 13, "_reads": 17}[entry]]
    args = [cands.ctypes.data, tb.ctypes.data, len(tb) - 1, tech, min_align_size, float(min_mapping_ratio), threads]
    if entry:
        args += [want] if min_cov is None else [want, int(min_cov), int(min_size)]
    else:
        args.insert(0, None)          # host_pac
    _chk(getattr(lib(), "mhip_cns_accept_templates" + entry)(ctx.h, vol.h, *args, *(C.byref(o) for o in outs)))
    a = _cns_take(acc, ACCEPTED_DTYPE, na.value)
    s = _cns_buffer(st, sb.value)              # the strings stay where the library put them (gigabytes at config 2: no copy)
    begin = _cns_take(tbeg, np.int64, len(tb))
    nw = int(begin[-1]) if len(begin) else 0
    plan = _cns_plan_out(seg, segb, win, nwin, er, erb, len(tb) - 1) if want & CNS_WANT_PLAN else None
    if plan is not None and want & CNS_WANT_PIECES:
        plan["piece_begin"] = _cns_take(pcb, np.int64, int(nwin.value) + 1)
        npc = int(plan["piece_begin"][-1]) if len(plan["piece_begin"]) else 0
        plan["pieces"] = _cns_buffer(pc, npc * PIECE_DTYPE.itemsize).view(PIECE_DTYPE)
    if plan is not None and want & CNS_WANT_POA:
        plan["cns_begin"] = _cns_take(cnb, np.int64, int(nwin.value) + 1)
        plan["cns"] = _cns_buffer(cn, int(plan["cns_begin"][-1]) if len(plan["cns_begin"]) else 0)
    out = (a, s, nj.value, _cns_buffer(tab, 4 * nw).view(TABLE_DTYPE), _cns_buffer(idn, nw), begin, plan)
    if entry != "_reads":
        return out
    if not want & CNS_WANT_READS:
        return out + (None,)
    read_begin = _cns_take(rdb, np.int64, len(tb))
    return out + (dict(reads=_cns_take(rd, READ_DTYPE, int(read_begin[-1]) if len(read_begin) else 0), read_begin=read_begin, seq=_cns_take(sq, np.uint8, sqb.value)),)


def cns_accept_templates_plan(ctx, vol, cands, tmpl_begin, tech, min_align_size, min_mapping_ratio, want, min_cov, min_size, threads=8):
    """cns_accept_templates_ex with CNS_WANT_PLAN allowed in `want`: the consensus plan of every template, computed on the device behind
    its table — effective ranges (get_effective_ranges), the segments consensus_worker would correct (runs of mat_cnt + ins_cnt >= min_cov
    of at least 0.95 * min_size positions inside an effective range) and per segment the windows meap_consensus_one_segment hands to the
    POA (anchor to next anchor, some position in between UNDS or FDEL).  The mecat2cns defaults: min_cov 6 / min_size 5000 (PacBio),
    6 / 2000 (nanopore).  -> cns_accept_templates_ex's tuple + a dict: segments [SEGMENT_DTYPE] in template order then ascending beg,
    seg_begin [templates + 1], windows [WINDOW_DTYPE] in segment order then ascending sb (segment s owns windows[win_begin: win_end]),
    eranges [k, 2], erange_begin [templates + 1]; None without CNS_WANT_PLAN.  With CNS_WANT_PLAN alone neither strings nor tables are
    copied from the device."""
    return _cns_accept("_plan", ctx, vol, cands, tmpl_begin, tech, min_align_size, min_mapping_ratio, want, min_cov, min_size, threads)


def debug_cns_plan(ctx, table, ident, table_begin, ranges, range_begin, tech, min_cov, min_size):
    """test hook: the plan's host range function and kernels on host-supplied tables.  table [TABLE_DTYPE] / ident [uint8] of all
    templates, template k at [table_begin[k], table_begin[k + 1]); ranges [m, 2] int32 (soff, send) of the accepted alignments, template
    k's at [range_begin[k], range_begin[k + 1]).  The ident bytes are taken as given.  -> the plan dict of cns_accept_templates_plan"""
    table = np.ascontiguousarray(table, dtype=TABLE_DTYPE)
    ident = np.ascontiguousarray(ident, dtype=np.uint8)
    tbeg = np.ascontiguousarray(table_begin, dtype=np.int64)
    rng = np.ascontiguousarray(ranges, dtype=np.int32).reshape(-1, 2)
    rbeg = np.ascontiguousarray(range_begin, dtype=np.int64)
    assert len(tbeg) == len(rbeg) >= 1 and len(table) == len(ident) == tbeg[-1] and len(rng) == rbeg[-1]
    seg, segb, win, er, erb = C.c_void_p(), C.c_void_p(), C.c_void_p(), C.c_void_p(), C.c_void_p()
    nwin = C.c_int64()
    _chk(lib().mhip_debug_cns_plan(ctx.h, table.ctypes.data, ident.ctypes.data, tbeg.ctypes.data, len(tbeg) - 1, rng.ctypes.data, rbeg.ctypes.data, int(tech),
                                   int(min_cov), int(min_size), C.byref(seg), C.byref(segb), C.byref(win), C.byref(nwin), C.byref(er), C.byref(erb)))
    return _cns_plan_out(seg, segb, win, nwin, er, erb, len(tbeg) - 1)


def debug_scan(ctx, cnt, base=0, n=None):
    """test hook: the single-workgroup scan (csrc/scan.h) through the plan's prefix-sum kernel.  cnt: int32 counts, n: how many of them
    (all).  -> int64 [n + 1], out[i] = base + cnt[0] + .. + cnt[i - 1]"""
    cnt = np.ascontiguousarray(cnt, dtype=np.int32)
    n = len(cnt) if n is None else int(n)
    assert n <= len(cnt)
    out = np.empty(max(n, 0) + 1, np.int64)
    _chk(lib().mhip_debug_scan(ctx.h, cnt.ctypes.data, n, int(base), out.ctypes.data))
    return out


CNS_WANT_PIECES = 8
PIECE_DTYPE = np.dtype([("aln", np.int32), ("col", np.int32), ("ncols", np.int32), ("sb_out", np.int32)])              # mhip_cns_piece
assert PIECE_DTYPE.itemsize == 16


def cns_accept_templates_pieces(ctx, vol, cands, tmpl_begin, tech, min_align_size, min_mapping_ratio, want, min_cov, min_size, threads=8):
    """cns_accept_templates_plan with CNS_WANT_PIECES allowed in `want` (it needs CNS_WANT_PLAN): what the reference hands to the POA for
    every listed window — CnsAln::retrieve_aln_subseqs of every accepted alignment of the template, in add order — as descriptors.  The
    plan dict gets two more entries: pieces [PIECE_DTYPE] and piece_begin [windows + 1]; window w owns pieces[piece_begin[w]:
    piece_begin[w + 1]], ascending `aln` (index into `accepted`).  A piece's substrings are qaln[col: col + ncols] and saln[col: col + ncols]
    of that record; the reference feeds them to the graph with addAln(qstr, tstr, sb_out - sb + 1).  Without CNS_WANT_PIECES the result
    is cns_accept_templates_plan's.  With CNS_WANT_PLAN | CNS_WANT_PIECES alone neither strings nor tables are copied from the device."""
    return _cns_accept("_pieces", ctx, vol, cands, tmpl_begin, tech, min_align_size, min_mapping_ratio, want, min_cov, min_size, threads)


def _cns_pairs_args(buf, off, lens, soff, send, windows, wstride):
    """-> (debug_cns_pieces' and debug_cns_poa's arguments behind the context, the arrays they point into)"""
    buf = np.ascontiguousarray(buf, dtype=np.uint8)
    off = np.ascontiguousarray(off, dtype=np.int64)
    lens, soff, send = (np.ascontiguousarray(x, dtype=np.int32) for x in (lens, soff, send))
    win = np.ascontiguousarray(windows, dtype=np.int32).reshape(-1, wstride)
    assert len(off) == len(lens) == len(soff) == len(send)
    return [buf.ctypes.data, len(buf), off.ctypes.data, lens.ctypes.data, soff.ctypes.data, send.ctypes.data, len(off), win.ctypes.data, len(win)], (buf, off, lens, soff, send, win)


def debug_cns_pieces(ctx, buf, off, lens, soff, send, windows):
    """test hook: the piece kernels on one template.  buf: uint8 buffer, pair p = qaln at off[p] (lens[p] characters + NUL), saln right
    behind it, with soff[p] / send[p]; windows [k, 2] int32 (sb, se), ascending and disjoint.  -> (pieces [PIECE_DTYPE], piece_begin
    [k + 1]); `aln` is the pair's number"""
    args, keep = _cns_pairs_args(buf, off, lens, soff, send, windows, 2)
    pc, pcb = C.c_void_p(), C.c_void_p()
    _chk(lib().mhip_debug_cns_pieces(ctx.h, *args, C.byref(pc), C.byref(pcb)))
    piece_begin = _cns_take(pcb, np.int64, len(keep[-1]) + 1)
    return _cns_take(pc, PIECE_DTYPE, int(piece_begin[-1])), piece_begin


CNS_WANT_POA = 16


def cns_poa_small_words():
    """the slot of cns_poa_small in 32-bit words (a window goes there when 17 * nodes + 8 * edges fits; see mecat_hip.h)"""
    return int(lib().mhip_cns_poa_small_words())


def cns_accept_templates_poa(ctx, vol, cands, tmpl_begin, tech, min_align_size, min_mapping_ratio, want, min_cov, min_size, threads=8):
    """cns_accept_templates_pieces with CNS_WANT_POA allowed in `want` (it needs CNS_WANT_PLAN): the POA consensus of every listed window,
    computed on the device — meap_cns_one_indel's `cns` (AlnGraphBoost: addAln of the window's pieces, mergeNodes, consensus at
    (int)(cov * 0.4)).  The plan dict gets two more entries: cns [uint8] and cns_begin [windows + 1]; window w owns cns[cns_begin[w]:
    cns_begin[w + 1]], both end letters included.  Without CNS_WANT_POA the result is cns_accept_templates_pieces'.  The pieces are
    copied from the device only with CNS_WANT_PIECES; CNS_WANT_PLAN | CNS_WANT_POA alone copies no strings, tables or pieces."""
    return _cns_accept("_poa", ctx, vol, cands, tmpl_begin, tech, min_align_size, min_mapping_ratio, want, min_cov, min_size, threads)


def debug_cns_poa(ctx, buf, off, lens, soff, send, windows):
    """test hook: the piece kernels and then the POA kernels on one template.  debug_cns_pieces' arguments with windows [k, 3] int32
    (sb, se, cov).  -> (cns [uint8], cns_begin [k + 1])"""
    args, keep = _cns_pairs_args(buf, off, lens, soff, send, windows, 3)
    cn, cnb = C.c_void_p(), C.c_void_p()
    _chk(lib().mhip_debug_cns_poa(ctx.h, *args, C.byref(cn), C.byref(cnb)))
    cns_begin = _cns_take(cnb, np.int64, len(keep[-1]) + 1)
    return _cns_take(cn, np.uint8, int(cns_begin[-1])), cns_begin


CNS_WANT_READS = 32
READ_DTYPE = np.dtype([("read_id", np.int32), ("range_beg", np.int32), ("range_end", np.int32), ("size", np.int32), ("seq_begin", np.int64),
                       ("template_index", np.int32), ("segment", np.int32)])                                            # mhip_cns_read
assert READ_DTYPE.itemsize == 32


def cns_accept_templates_reads(ctx, vol, cands, tmpl_begin, tech, min_align_size, min_mapping_ratio, want, min_cov, min_size, threads=8):
    """cns_accept_templates_poa with CNS_WANT_READS allowed in `want`, alone or with any other bit: the corrected reads, assembled on the
    device behind the POA — every segment's target (the anchors' letters and the inner letters of the listed windows' consensus), the
    min_size filter and output_cns_result's records.  -> cns_accept_templates_poa's tuple + a dict (None without the bit): reads
    [READ_DTYPE] (template t owns reads[read_begin[t]: read_begin[t + 1]], in segment order then block order; record r owns
    seq[seq_begin: seq_begin + size]), read_begin [templates + 1], seq [uint8].  With the bit the table, plan, pieces and POA are computed
    on the device whether or not their bits are set and copied only with them; CNS_WANT_READS alone copies the accepted records and the
    reads."""
    return _cns_accept("_reads", ctx, vol, cands, tmpl_begin, tech, min_align_size, min_mapping_ratio, want, min_cov, min_size, threads)


def cns_format_reads(reads, seq):
    """the reference's text of the records (reads_correction_can.cpp:44-46): '>' id '_' range0 '_' range1 '_' size, newline, letters,
    newline -> bytes"""
    reads = np.ascontiguousarray(reads, dtype=READ_DTYPE)
    seq = np.ascontiguousarray(seq, dtype=np.uint8)
    text, n = C.c_void_p(), C.c_int64()
    _chk(lib().mhip_cns_format_reads(reads.ctypes.data, len(reads), seq.ctypes.data, len(seq), C.byref(text), C.byref(n)))
    return _cns_take(text, np.uint8, n.value).tobytes()


CNS_WANT_TEXT = 64


def cns_correct_templates(ctx, vol, cands, tmpl_begin, tech, min_align_size, min_mapping_ratio, want, min_cov, min_size, input_type=0, threads=8):
    """mhip_cns_correct_templates: cns_accept_templates_reads with the options and outputs in structs, CNS_WANT_TEXT allowed in `want`
    (the reference's FASTA text of the records, made on the device; alone it copies the accepted records and the text, nothing else) and
    input_type 1 for the m4 walk (a template's records are overlaps in the order given; see mecat_hip.h).  -> (the tuple of
    cns_accept_templates_reads, the text as bytes or None without the bit, cands as the call left them, and per pointer member of the
    outputs whether it came back NULL)"""
    cands = np.array(cands, copy=True)
    tb = np.ascontiguousarray(tmpl_begin, dtype=np.int64)
    want = int(want)
    nt = len(tb) - 1
    o = CnsOpts(int(tech), int(input_type), int(min_align_size), int(min_cov), int(min_size), int(threads), want, float(min_mapping_ratio))
    r = CnsOutputs()
    _chk(lib().mhip_cns_correct_templates(ctx.h, vol.h, cands.ctypes.data, tb.ctypes.data, nt, C.byref(o), C.byref(r)))
    null = {k: getattr(r, k) is None for k, t in CnsOutputs._fields_ if t is C.c_void_p}
    def take(name, dtype, n):      # a copy of the member's records; the member is released and cleared
        x = _cns_take(C.c_void_p(getattr(r, name)), dtype, n)
        setattr(r, name, None)
        return x
    a = take("accepted", ACCEPTED_DTYPE, r.count)
    s = take("strings", np.uint8, r.strings_bytes)
    begin = take("table_begin", np.int64, nt + 1)
    nw = int(begin[-1]) if len(begin) else 0
    tab, idn = take("table", np.uint8, 4 * nw).view(TABLE_DTYPE), take("ident", np.uint8, nw)
    plan = None
    if want & CNS_WANT_PLAN:
        segb, erb = take("seg_begin", np.int64, nt + 1), take("erange_begin", np.int64, nt + 1)
        plan = dict(segments=take("segments", SEGMENT_DTYPE, int(segb[-1]) if len(segb) else 0), seg_begin=segb,
                    windows=take("windows", WINDOW_DTYPE, int(r.n_windows)),
                    eranges=take("eranges", np.int32, 2 * (int(erb[-1]) if len(erb) else 0)).reshape(-1, 2), erange_begin=erb)
        if want & CNS_WANT_PIECES:
            plan["piece_begin"] = take("piece_begin", np.int64, int(r.n_windows) + 1)
            plan["pieces"] = take("pieces", PIECE_DTYPE, int(plan["piece_begin"][-1]) if len(plan["piece_begin"]) else 0)
        if want & CNS_WANT_POA:
            plan["cns_begin"] = take("cns_begin", np.int64, int(r.n_windows) + 1)
            plan["cns"] = take("cns", np.uint8, int(plan["cns_begin"][-1]) if len(plan["cns_begin"]) else 0)
    rd = None
    if want & CNS_WANT_READS:
        rb = take("read_begin", np.int64, nt + 1)
        rd = dict(reads=take("reads", READ_DTYPE, int(rb[-1]) if len(rb) else 0), read_begin=rb, seq=take("seq", np.uint8, r.seq_bytes))
    text = take("text", np.uint8, r.text_bytes).tobytes() if want & CNS_WANT_TEXT else None
    jobs = r.jobs
    lib().mhip_cns_outputs_free(C.byref(r))      # (whatever the wanted bits did not take)
    return (a, s, jobs, tab, idn, begin, plan, rd), text, cands, null


def debug_cns_text(ctx, reads, seq):
    """test hook: the text kernels alone on host-supplied records (see mecat_hip.h) -> bytes"""
    reads = np.ascontiguousarray(reads, dtype=READ_DTYPE)
    seq = np.ascontiguousarray(seq, dtype=np.uint8)
    text, n = C.c_void_p(), C.c_int64()
    _chk(lib().mhip_debug_cns_text(ctx.h, reads.ctypes.data, len(reads), seq.ctypes.data, len(seq), C.byref(text), C.byref(n)))
    return _cns_take(text, np.uint8, n.value).tobytes()


def debug_cns_reads(ctx, table, ident, table_begin, read_ids, segments, windows, cns, cns_begin, min_size):
    """test hook: the read kernels alone on host-supplied arrays (see mecat_hip.h).  -> dict(reads, read_begin, seq)"""
    table = np.ascontiguousarray(table, dtype=TABLE_DTYPE)
    ident = np.ascontiguousarray(ident, dtype=np.uint8)
    tbeg = np.ascontiguousarray(table_begin, dtype=np.int64)
    rid = np.ascontiguousarray(read_ids, dtype=np.int32)
    seg = np.ascontiguousarray(segments, dtype=SEGMENT_DTYPE)
    win = np.ascontiguousarray(windows, dtype=WINDOW_DTYPE)
    cns = np.ascontiguousarray(cns, dtype=np.uint8)
    cb = np.ascontiguousarray(cns_begin, dtype=np.int64)
    assert len(tbeg) >= 1 and len(table) == len(ident) == tbeg[-1] and len(rid) == len(tbeg) - 1 and len(cb) == len(win) + 1 and len(cns) >= cb[-1]
    rd, rdb, sq = C.c_void_p(), C.c_void_p(), C.c_void_p()
    sqb = C.c_int64()
    _chk(lib().mhip_debug_cns_reads(ctx.h, table.ctypes.data, ident.ctypes.data, tbeg.ctypes.data, len(tbeg) - 1, rid.ctypes.data, seg.ctypes.data, len(seg), win.ctypes.data,
                                    len(win), cns.ctypes.data, cb.ctypes.data, int(min_size), C.byref(rd), C.byref(rdb), C.byref(sq), C.byref(sqb)))
    read_begin = _cns_take(rdb, np.int64, len(tbeg))
    return dict(reads=_cns_take(rd, READ_DTYPE, int(read_begin[-1])), read_begin=read_begin, seq=_cns_take(sq, np.uint8, sqb.value))


def debug_cns_correct(ctx, buf, off, lens, soff, send, tmpl_letters, tech, min_cov, min_size, read_id):
    """test hook: the whole back end on one template — table, plan, pieces, POA, reads — through the accept stage's launchers.  The
    alignments as debug_cns_pieces takes them, the template's letters as bytes.  -> (reads [READ_DTYPE], seq [uint8])"""
    buf = np.ascontiguousarray(buf, dtype=np.uint8)
    off = np.ascontiguousarray(off, dtype=np.int64)
    lens, soff, send = (np.ascontiguousarray(x, dtype=np.int32) for x in (lens, soff, send))
    let = np.frombuffer(bytes(tmpl_letters), dtype=np.uint8)
    assert len(off) == len(lens) == len(soff) == len(send)
    rd, sq = C.c_void_p(), C.c_void_p()
    nr, sqb = C.c_int64(), C.c_int64()
    _chk(lib().mhip_debug_cns_correct(ctx.h, buf.ctypes.data, len(buf), off.ctypes.data, lens.ctypes.data, soff.ctypes.data, send.ctypes.data, len(off), let.ctypes.data,
                                      len(let), int(tech), int(min_cov), int(min_size), int(read_id), C.byref(rd), C.byref(nr), C.byref(sq), C.byref(sqb)))
    return _cns_take(rd, READ_DTYPE, nr.value), _cns_take(sq, np.uint8, sqb.value)


COMM_ID_BYTES = 128
SHARD_CHUNK = 500


def comm_unique_id():
    """rank 0: the RCCL unique id (bytes) to hand to every rank"""
    buf = (C.c_uint8 * COMM_ID_BYTES)()
    _chk(lib().mhip_comm_unique_id(buf))
    return bytes(buf)


class Comm:
    """mhip_comm: RCCL communicator over one context per rank (hostfile_dir: the test-hook transport)"""

    def __init__(self, ctx, nranks, rank, unique_id=None, hostfile_dir=None, run_id="0", solo=False):
        self.h = C.c_void_p()
        self.ctx, self.nranks, self.rank = ctx, nranks, rank
        if solo:        # bench hook: this rank's share of every sharded call, no transport (mecat_hip.h: mhip_comm_init_solo)
            lib().mhip_comm_init_solo.argtypes = [C.c_void_p, C.c_int, C.c_int, C.POINTER(C.c_void_p)]
            _chk(lib().mhip_comm_init_solo(ctx.h, nranks, rank, C.byref(self.h)))
        elif hostfile_dir is not None:
            _chk(lib().mhip_comm_init_hostfile(ctx.h, nranks, rank, hostfile_dir.encode(), run_id.encode(), C.byref(self.h)))
        else:
            buf = (C.c_uint8 * COMM_ID_BYTES).from_buffer_copy(unique_id if unique_id is not None else bytes(COMM_ID_BYTES))
            _chk(lib().mhip_comm_init(ctx.h, nranks, rank, buf, C.byref(self.h)))

    def close(self):
        if self.h:
            lib().mhip_comm_destroy(self.h)
            self.h = C.c_void_p()

    def barrier(self):
        _chk(lib().mhip_comm_barrier(self.h))

    def info(self):
        """-> (transport: 0 RCCL / 1 host files, ncclCommCount of the RCCL communicator)"""
        t, n = C.c_int(), C.c_int()
        _chk(lib().mhip_comm_info(self.h, C.byref(t), C.byref(n)))
        return t.value, n.value

    def bytes_sent(self):
        lib().mhip_comm_bytes_sent.restype = C.c_int64
        lib().mhip_comm_bytes_sent.argtypes = [C.c_void_p]
        return int(lib().mhip_comm_bytes_sent(self.h))

    def local_jobs(self):
        lib().mhip_comm_local_jobs.restype = C.c_int64
        lib().mhip_comm_local_jobs.argtypes = [C.c_void_p]
        return int(lib().mhip_comm_local_jobs(self.h))

    def bytes_received(self):
        return int(lib().mhip_comm_bytes_received(self.h))

    def index_build_sharded(self, vol):
        """mhip_index_build_sharded: the volume's table built by all ranks together; every rank gets the complete table"""
        idx = Index.__new__(Index)
        idx.h = C.c_void_p()
        idx.ctx = self.ctx
        lib().mhip_index_build_sharded.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(C.c_void_p)]
        _chk(lib().mhip_index_build_sharded(self.h, vol.h, C.byref(idx.h)))
        return idx

    def index_build_auto(self, vol):
        """mhip_index_build_auto: the faster of Index(ctx, vol) on every rank and index_build_sharded, measured by the first call on this
        communicator.  -> (index, {"replicated_ms", "sharded_ms", "chosen"})"""
        idx = Index.__new__(Index)
        idx.h = C.c_void_p()
        idx.ctx = self.ctx
        ms = (C.c_double * 2)()
        sh = C.c_int()
        lib().mhip_index_build_auto.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_double), C.POINTER(C.c_int)]
        _chk(lib().mhip_index_build_auto(self.h, vol.h, C.byref(idx.h), ms, C.byref(sh)))
        return idx, {"replicated_ms": ms[0], "sharded_ms": ms[1], "chosen": "sharded" if sh.value else "replicated",
                     "measured": ms[0] > 0 or ms[1] > 0}

    def seed_reads_sharded(self, idx, ref, reads, rid_begin, rid_end, params, chunk=SHARD_CHUNK, cell_shift=0, host=True):
        """-> (cands [n, maxc] structured, counts [n]) on the host when host=True, else None (tables stay on the device)"""
        n = rid_end - rid_begin
        if host:
            out = np.zeros((n, params.maxc), dtype=CAND_DTYPE)
            cnt = np.zeros(n, dtype=np.int32)
            _chk(lib().mhip_seed_reads_sharded(self.h, idx.h, ref.h, reads.h, rid_begin, rid_end, chunk, cell_shift, C.byref(params),
                                               out.ctypes.data, cnt.ctypes.data))
            return out, cnt
        _chk(lib().mhip_seed_reads_sharded(self.h, idx.h, ref.h, reads.h, rid_begin, rid_end, chunk, cell_shift, C.byref(params), None, None))
        return None

    def align_sharded(self, ref, reads, min_align_size, tech=0, host=True):
        """-> results of every candidate of the slab, read-major (host=True), and their number"""
        nj = C.c_int64()
        if not host:
            _chk(lib().mhip_align_sharded(self.h, ref.h, reads.h, tech, min_align_size, None, C.byref(nj)))
            return None, nj.value
        _, _, _, total = self.tables()
        out = np.zeros(max(total, 1), dtype=ALN_DTYPE)
        _chk(lib().mhip_align_sharded(self.h, ref.h, reads.h, tech, min_align_size, out.ctypes.data, C.byref(nj)))
        return out[: nj.value], nj.value

    def tables(self):
        """device pointers (cands, counts, results) of the last sharded calls and the number of jobs"""
        a, b, c2, nj = C.c_void_p(), C.c_void_p(), C.c_void_p(), C.c_int64()
        _chk(lib().mhip_sharded_tables(self.h, C.byref(a), C.byref(b), C.byref(c2), C.byref(nj)))
        return a.value, b.value, c2.value, nj.value
