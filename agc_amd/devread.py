"""A sample's FASTA text written on the GPU: the host reader opens the archive and decodes the zstd parts (agc_amd/reader.py,
libagc_read.so), everything behind that -- the LZ-diff decode, orientation, the k-symbol overlap, the alphabet and the line
wrapping -- is one call of the device library (include/agc_hip.h: agc_hip_sample_fasta).

    ctx = capi.Context(0)
    r = DeviceReader(ctx, "collection.agc")
    text = r.sample_fasta("HG00438.1")          # bytes, what `agc getset` writes
    d = r.sample_fasta_dev("HG00438.1")         # the same as a torch uint8 tensor on the device
    r.close()

Group references are registered with the context once, as gid_base + group id: two readers on one context need disjoint ranges.
There is no host fallback: without a device the context cannot be made."""
import ctypes as C

import numpy as np

from agc_amd import capi, reader


class DeviceReader:
    def __init__(self, ctx, path, gid_base=0):
        self.ctx = ctx
        self.gid_base = int(gid_base)
        self.file = reader.CAGCFile()
        if not self.file.Open(path):
            raise RuntimeError(f"{path}: not a readable .agc archive")
        prm = self.file.GetParams()
        self.k, self.min_match_len = prm["k"], prm["min_match_len"]
        self.registered = set()
        self._pinned, self._pinned_cap = None, 0

    def close(self):
        if self.file is not None:
            self.file.Close()
            self.file = None

    def plan(self, name):
        """the sample's plan (reader.CAGCFile.GetSamplePlan) with its new references registered -> the arguments of Context.sample_fasta"""
        if self.file is None:
            raise RuntimeError("the reader is closed")
        p = self.file.GetSamplePlan(name)
        if p is None:
            raise KeyError(name)
        for i, g in enumerate(p["groups"].tolist()):
            if g not in self.registered:
                self.ctx.ref_register(self.gid_base + g, p["ref_bytes"][int(p["ref_off"][i]):int(p["ref_off"][i + 1])], self.min_match_len)
                self.registered.add(g)
        segs = np.zeros(p["kind"].size, capi.SEG_SRC_DTYPE)
        segs["kind"] = p["kind"]  # (reader.PLAN_* and capi.SEG_* are the same numbers)
        segs["gid"] = np.where(p["kind"] == capi.SEG_RAW, 0, p["group_id"] + np.uint32(self.gid_base))
        segs["off"], segs["n_bytes"], segs["length"], segs["rc"] = p["off"], p["seg_bytes"], p["length"], p["rc"]
        return p["ctg_seg"], segs, p["bytes"], p["names"], p["name_off"]

    def _pinned_buffer(self, n):
        if n > self._pinned_cap:
            if self._pinned is not None:
                self.ctx._chk(self.ctx.L.agc_hip_host_free(self.ctx.h, self._pinned))
            cap = n + n // 4 + 4096
            self._pinned, self._pinned_cap = self.ctx.host_alloc(cap), cap
        return self._pinned

    def sample_fasta(self, name, line_length=80):
        """-> bytes: the sample as `agc getset` writes it (line_length 0: one line per contig)"""
        ctg_seg, segs, data, names, name_off = self.plan(name)
        L = self.ctx.L.agc_hip_sample_fasta
        rc, need = self.ctx.sample_fasta_raw(L, ctg_seg, segs, data, self.k, line_length, names, name_off, self._pinned, self._pinned_cap)
        if rc == capi.ECAP:  # (the text's size follows from the plan: nothing was launched)
            rc, need = self.ctx.sample_fasta_raw(L, ctg_seg, segs, data, self.k, line_length, names, name_off, self._pinned_buffer(need), self._pinned_cap)
        self.ctx._chk(rc)
        return C.string_at(self._pinned, need) if need else b""

    def sample_fasta_dev(self, name, line_length=80):
        """-> the same text as a torch uint8 tensor on the context's device"""
        import torch
        ctg_seg, segs, data, names, name_off = self.plan(name)
        rc, need = self.ctx.sample_fasta_raw(self.ctx.L.agc_hip_sample_fasta_dev, ctg_seg, segs, data, self.k, line_length, names, name_off, None, 0)
        if rc != capi.ECAP:
            self.ctx._chk(rc)
        out = torch.empty(need, dtype=torch.uint8, device="cuda")
        if need:
            torch.cuda.synchronize()
            self.ctx.sample_fasta_dev(ctg_seg, segs, data, self.k, line_length, names, name_off, out.data_ptr(), need)
        return out
