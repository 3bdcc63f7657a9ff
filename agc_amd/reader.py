"""ctypes binding of the read side (libagc_read.so, include/agc_read.h).

`CAGCFile` mirrors the class the reference exports to Python (src/py_agc_api/py_agc_api.cpp:28-84: Open, Close,
NSample, GetReferenceSample, NCtg, ListSample, ListCtg, GetCtgLen, GetCtgSeq with and without a sample name), so
src/py_agc_api/py_agc_test.py reads the same against this module (`StringVector` is a plain list here).
Host code only -- no torch, no HIP."""
import ctypes as C
import os

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(HERE, "libagc_read.so")
SYMBOLS = ["agc_open", "agc_close", "agc_get_ctg_len", "agc_get_ctg_seq", "agc_n_sample", "agc_n_ctg", "agc_reference_sample",
           "agc_list_sample", "agc_list_ctg", "agc_list_destroy", "agc_string_destroy", "agc_get_sample_fasta", "agc_get_params",
           "agc_get_sample_plan", "agc_plan_fields", "agc_plan_destroy", "agc_get_sample_parts", "agc_parts_fields", "agc_parts_destroy",
           "agc_get_range_parts", "agc_ranges_fields", "agc_ranges_destroy"]
PLAN_RAW, PLAN_REF, PLAN_DELTA = 0, 1, 2
PART_STORED, PART_ZSTD = 0, 1
PART_PACK, PART_REF_BYTES, PART_REF_TUPLES = 0, 1, 2


class PlanView(C.Structure):
    """agc_plan_view (include/agc_read.h)"""
    _u32p, _u64p = C.POINTER(C.c_uint32), C.POINTER(C.c_uint64)
    _fields_ = [("n_ctg", C.c_uint64), ("n_seg", C.c_uint64), ("n_bytes", C.c_uint64), ("n_groups", C.c_uint64),
                ("names", C.c_void_p), ("name_off", _u64p), ("ctg_seg", _u64p),
                ("group_id", _u32p), ("in_group_id", _u32p), ("rc", _u32p), ("length", _u32p), ("kind", _u32p), ("seg_bytes", _u32p),
                ("off", _u64p), ("bytes", C.c_void_p), ("groups", _u32p), ("ref_off", _u64p), ("ref_bytes", C.c_void_p)]


class PartsView(C.Structure):
    """agc_parts_view (include/agc_read.h)"""
    _u32p, _u64p = C.POINTER(C.c_uint32), C.POINTER(C.c_uint64)
    _fields_ = [("n_ctg", C.c_uint64), ("n_seg", C.c_uint64), ("n_parts", C.c_uint64), ("src_bytes", C.c_uint64), ("src", C.c_void_p),
                ("names", C.c_void_p), ("name_off", _u64p), ("ctg_seg", _u64p),
                ("group_id", _u32p), ("in_group_id", _u32p), ("rc", _u32p), ("length", _u32p), ("kind", _u32p), ("seg_part", _u32p), ("seg_index", _u32p),
                ("part_off", _u64p), ("part_bytes", _u32p), ("part_coding", _u32p), ("part_content", _u32p), ("part_group", _u32p), ("part_no", _u32p)]


class RangesView(C.Structure):
    """agc_ranges_view (include/agc_read.h)"""
    _u32p, _u64p = C.POINTER(C.c_uint32), C.POINTER(C.c_uint64)
    _fields_ = [("n_q", C.c_uint64), ("n_win", C.c_uint64), ("n_parts", C.c_uint64), ("src_bytes", C.c_uint64), ("src", C.c_void_p),
                ("q_seg", _u64p), ("q_len", _u64p),
                ("group_id", _u32p), ("in_group_id", _u32p), ("rc", _u32p), ("length", _u32p), ("kind", _u32p), ("seg_part", _u32p), ("seg_index", _u32p),
                ("win_from", _u32p), ("win_len", _u32p),
                ("part_off", _u64p), ("part_bytes", _u32p), ("part_coding", _u32p), ("part_content", _u32p), ("part_group", _u32p), ("part_no", _u32p)]


_lib = None


def _arr(ptr, n, dt):
    """n items of type dt at ptr (an address or a ctypes pointer) as a numpy array of its own"""
    import numpy as np
    n = int(n)
    if not n:
        return np.zeros(0, dt)
    addr = ptr if isinstance(ptr, int) else C.addressof(ptr.contents)
    return np.frombuffer((C.c_char * (n * np.dtype(dt).itemsize)).from_address(addr), dtype=dt).copy()


def load():
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(f"{LIB_PATH} is missing: run `python -m agc_amd.build`")
    L = C.CDLL(LIB_PATH)
    vp, cp, ci = C.c_void_p, C.c_char_p, C.c_int
    L.agc_open.restype = vp
    L.agc_open.argtypes = [cp, ci]
    L.agc_close.argtypes = [vp]
    L.agc_get_ctg_len.argtypes = [vp, cp, cp]
    L.agc_get_ctg_seq.argtypes = [vp, cp, cp, ci, ci, cp]
    L.agc_n_sample.argtypes = [vp]
    L.agc_n_ctg.argtypes = [vp, cp]
    L.agc_reference_sample.restype = vp
    L.agc_reference_sample.argtypes = [vp]
    L.agc_list_sample.restype = C.POINTER(vp)
    L.agc_list_sample.argtypes = [vp, C.POINTER(ci)]
    L.agc_list_ctg.restype = C.POINTER(vp)
    L.agc_list_ctg.argtypes = [vp, cp, C.POINTER(ci)]
    L.agc_list_destroy.argtypes = [C.POINTER(vp)]
    L.agc_string_destroy.argtypes = [vp]
    L.agc_get_sample_fasta.restype = vp
    L.agc_get_sample_fasta.argtypes = [vp, cp, ci, C.POINTER(C.c_longlong)]
    L.agc_get_params.argtypes = [vp] + [C.POINTER(C.c_uint)] * 4
    L.agc_get_sample_plan.restype = vp
    L.agc_get_sample_plan.argtypes = [vp, cp]
    L.agc_plan_fields.argtypes = [vp, C.POINTER(PlanView)]
    L.agc_plan_destroy.argtypes = [vp]
    L.agc_get_sample_parts.restype = vp
    L.agc_get_sample_parts.argtypes = [vp, cp, C.POINTER(C.c_uint32), C.c_uint64]
    L.agc_parts_fields.argtypes = [vp, C.POINTER(PartsView)]
    L.agc_parts_destroy.argtypes = [vp]
    L.agc_get_range_parts.restype = vp
    L.agc_get_range_parts.argtypes = [vp, C.c_uint64, C.POINTER(cp), C.POINTER(cp), C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.POINTER(C.c_uint32), C.c_uint64,
                                      C.POINTER(C.c_int64)]
    L.agc_ranges_fields.argtypes = [vp, C.POINTER(RangesView)]
    L.agc_ranges_destroy.argtypes = [vp]
    _lib = L
    return L


class StringVector(list):
    """stand-in for py_agc_api.StringVector (py_agc_api.cpp:18-26)"""


class CAGCFile:
    def __init__(self):
        self.L = load()
        self.h = None

    def Open(self, file_name, prefetching=True):
        if self.h:
            return False
        self.h = self.L.agc_open(os.fsencode(file_name), 1 if prefetching else 0)
        return bool(self.h)

    def Close(self):
        if not self.h:
            return False
        r = self.L.agc_close(self.h)
        self.h = None
        return r == 0

    def __del__(self):
        if getattr(self, "h", None):
            self.Close()

    def NSample(self):
        return self.L.agc_n_sample(self.h) if self.h else -1

    def NCtg(self, sample):
        return self.L.agc_n_ctg(self.h, sample.encode()) if self.h else -1

    def GetReferenceSample(self):
        if not self.h:
            return ""
        p = self.L.agc_reference_sample(self.h)
        if not p:
            return ""
        s = C.string_at(p).decode()
        self.L.agc_string_destroy(p)
        return s

    def _list(self, arr, n, out):
        names = [C.string_at(arr[i]).decode() for i in range(n)] if arr else []
        if arr:
            self.L.agc_list_destroy(arr)
        if out is not None:
            del out[:]
            out.extend(names)
            return 0
        return names

    def ListSample(self, out=None):
        if not self.h:
            return -1
        n = C.c_int(0)
        return self._list(self.L.agc_list_sample(self.h, C.byref(n)), n.value, out)

    def ListCtg(self, sample, out=None):
        if not self.h:
            return -1
        n = C.c_int(0)
        return self._list(self.L.agc_list_ctg(self.h, sample.encode(), C.byref(n)), n.value, out)

    def GetCtgLen(self, sample, name):
        if not self.h:
            return -1
        return self.L.agc_get_ctg_len(self.h, sample.encode() if sample else None, name.encode())

    def GetCtgSeq(self, *args):
        """GetCtgSeq(sample, name, start, end) or GetCtgSeq(name, start, end); [start, end] inclusive, -1/-1 = all"""
        if len(args) == 3:
            sample, (name, start, end) = "", args
        else:
            sample, name, start, end = args
        if not self.h:
            return ""
        n = self.GetCtgLen(sample, name)
        if n < 0:
            return ""
        buf = C.create_string_buffer(n + 1)
        r = self.L.agc_get_ctg_seq(self.h, sample.encode() if sample else None, name.encode(), start, end, buf)
        return buf.raw[:r].decode() if r >= 0 else ""

    # extensions
    def GetSampleFasta(self, sample, line_length=80):
        n = C.c_longlong(0)
        p = self.L.agc_get_sample_fasta(self.h, sample.encode(), line_length, C.byref(n))
        if not p:
            return None
        s = C.string_at(p, n.value)
        self.L.agc_string_destroy(p)
        return s

    def GetParams(self):
        v = [C.c_uint(0) for _ in range(4)]
        if self.L.agc_get_params(self.h, *[C.byref(x) for x in v]) != 0:
            return None
        return dict(zip(("k", "min_match_len", "pack_cardinality", "segment_size"), (x.value for x in v)))

    def GetSamplePlan(self, sample):
        """the plan of a whole sample (agc_get_sample_plan) as numpy arrays of their own, or None for an unknown sample:
        names (bytes) / name_off, ctg_seg, per segment group_id / in_group_id / rc / length / kind (PLAN_*) / seg_bytes / off, the
        byte blob `bytes` the RAW and DELTA segments name, groups (>= 16, ascending) with ref_off / ref_bytes"""
        import numpy as np
        h = self.L.agc_get_sample_plan(self.h, sample.encode()) if self.h else None
        if not h:
            return None
        try:
            v = PlanView()
            if self.L.agc_plan_fields(h, C.byref(v)) != 0:
                return None
            arr = _arr

            out = {"name_off": arr(v.name_off, v.n_ctg + 1, np.uint64), "ctg_seg": arr(v.ctg_seg, v.n_ctg + 1, np.uint64)}
            out["names"] = arr(v.names, out["name_off"][-1], np.uint8).tobytes()
            for f in ("group_id", "in_group_id", "rc", "length", "kind", "seg_bytes"):
                out[f] = arr(getattr(v, f), v.n_seg, np.uint32)
            out["off"] = arr(v.off, v.n_seg, np.uint64)
            out["bytes"] = arr(v.bytes, v.n_bytes, np.uint8)
            out["groups"] = arr(v.groups, v.n_groups, np.uint32)
            out["ref_off"] = arr(v.ref_off, v.n_groups + 1, np.uint64)
            out["ref_bytes"] = arr(v.ref_bytes, out["ref_off"][-1], np.uint8)
            return out
        finally:
            self.L.agc_plan_destroy(h)

    def GetSampleParts(self, sample, have=()):
        """the stored parts of a whole sample (agc_get_sample_parts) as numpy arrays of their own, or None for an unknown sample: names /
        name_off, ctg_seg, per segment group_id / in_group_id / rc / length / kind (PLAN_*) / seg_part / seg_index, per part part_off /
        part_bytes / part_coding (PART_STORED, PART_ZSTD) / part_content (PART_PACK, PART_REF_*) / part_group / part_no.  have: the
        groups whose references the caller has already.  src / src_bytes: the address and size of the archive's bytes the parts lie
        in -- the archive's own, valid until Close; part(i) copies one part out"""
        import numpy as np
        hv = np.ascontiguousarray(sorted(int(g) for g in have), dtype=np.uint32)
        h = self.L.agc_get_sample_parts(self.h, sample.encode(), hv.ctypes.data_as(C.POINTER(C.c_uint32)), hv.size) if self.h else None
        if not h:
            return None
        try:
            v = PartsView()
            if self.L.agc_parts_fields(h, C.byref(v)) != 0:
                return None
            arr = _arr

            out = {"name_off": arr(v.name_off, v.n_ctg + 1, np.uint64), "ctg_seg": arr(v.ctg_seg, v.n_ctg + 1, np.uint64)}
            out["names"] = arr(v.names, out["name_off"][-1], np.uint8).tobytes()
            for f in ("group_id", "in_group_id", "rc", "length", "kind", "seg_part", "seg_index"):
                out[f] = arr(getattr(v, f), v.n_seg, np.uint32)
            out["part_off"] = arr(v.part_off, v.n_parts, np.uint64)
            for f in ("part_bytes", "part_coding", "part_content", "part_group", "part_no"):
                out[f] = arr(getattr(v, f), v.n_parts, np.uint32)
            out["src"], out["src_bytes"] = v.src, int(v.src_bytes)
            out["part"] = lambda i: C.string_at(out["src"] + int(out["part_off"][i]), int(out["part_bytes"][i]))
            return out
        finally:
            self.L.agc_parts_destroy(h)

    def GetRangeParts(self, queries, have=()):
        """the windows and stored parts of a batch of contig ranges (agc_get_range_parts) as numpy arrays of their own.  queries: a
        sequence of (sample, contig, start, end) -- sample None or "": the contig name must be unique; the range as GetCtgSeq reads it.
        -> q_seg (n_q + 1) / q_len (n_q), per window entry group_id / in_group_id / rc / length / kind (PLAN_*) / seg_part / seg_index
        / win_from / win_len, the parts and src / src_bytes / part(i) as GetSampleParts has them (each part once for the whole batch).
        An unknown or ambiguous contig raises KeyError(the index of the first such query, the query)"""
        import numpy as np
        if not self.h:
            return None
        qs = list(queries)
        n = len(qs)
        smp = (C.c_char_p * max(n, 1))(*[q[0].encode() if q[0] else None for q in qs])
        nam = (C.c_char_p * max(n, 1))(*[q[1].encode() for q in qs])
        frm = np.ascontiguousarray([int(q[2]) for q in qs], dtype=np.int64)
        to = np.ascontiguousarray([int(q[3]) for q in qs], dtype=np.int64)
        hv = np.ascontiguousarray(sorted(int(g) for g in have), dtype=np.uint32)
        bad = C.c_int64(-1)
        i64p = C.POINTER(C.c_int64)
        h = self.L.agc_get_range_parts(self.h, n, smp, nam, frm.ctypes.data_as(i64p), to.ctypes.data_as(i64p), hv.ctypes.data_as(C.POINTER(C.c_uint32)), hv.size,
                                       C.byref(bad))
        if not h:
            if bad.value >= 0:
                raise KeyError(bad.value, tuple(qs[bad.value]))
            return None
        try:
            v = RangesView()
            if self.L.agc_ranges_fields(h, C.byref(v)) != 0:
                return None
            out = {"q_seg": _arr(v.q_seg, v.n_q + 1, np.uint64), "q_len": _arr(v.q_len, v.n_q, np.uint64)}
            for f in ("group_id", "in_group_id", "rc", "length", "kind", "seg_part", "seg_index", "win_from", "win_len"):
                out[f] = _arr(getattr(v, f), v.n_win, np.uint32)
            out["part_off"] = _arr(v.part_off, v.n_parts, np.uint64)
            for f in ("part_bytes", "part_coding", "part_content", "part_group", "part_no"):
                out[f] = _arr(getattr(v, f), v.n_parts, np.uint32)
            out["src"], out["src_bytes"] = v.src, int(v.src_bytes)
            out["part"] = lambda i: C.string_at(out["src"] + int(out["part_off"][i]), int(out["part_bytes"][i]))
            return out
        finally:
            self.L.agc_ranges_destroy(h)
