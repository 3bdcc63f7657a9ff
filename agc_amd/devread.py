"""A sample's FASTA text, and batches of contig ranges, written on the GPU.  A sample's text has two ways in, the same text out:

sample_fasta / sample_fasta_dev: the host reader opens the archive and decodes the zstd parts (agc_amd/reader.py, libagc_read.so),
everything behind that -- the LZ-diff decode, orientation, the k-symbol overlap, the alphabet and the line wrapping -- is one call
of the device library (include/agc_hip.h: agc_hip_sample_fasta).

sample_fasta_parts / sample_fasta_parts_dev: the host reader only reads the collection metadata and says which stored parts the
sample needs (GetSampleParts); their bytes go to the device as the archive holds them and are zstd-decoded, cut into sequences,
un-tupled and -- the references not registered yet -- registered there (agc_hip_sample_fasta_parts).

sample_fasta_bgzf / sample_fasta_bgzf_dev: the parts path with the text compressed where it is made -- BGZF, block deflate with
dynamic Huffman codes (agc_hip_sample_fasta_parts_bgzf) -- so that a third of the bytes cross to the host.

ranges / ranges_dev: a batch of windows (sample, contig, start, end) -- the range as GetCtgSeq reads it: inclusive, -1 / -1 the whole
contig -- through the same parts path: the host reader says which segments each range touches, which window of each, and which
stored parts the whole batch needs (GetRangeParts); the device decodes those parts and writes every window straight to its place
(agc_hip_ranges_parts).  No whole segment and no whole sample is materialised.

    ctx = capi.Context(0)
    r = DeviceReader(ctx, "collection.agc")
    text = r.sample_fasta("HG00438.1")          # bytes, what `agc getset` writes
    d = r.sample_fasta_dev("HG00438.1")         # the same as a torch uint8 tensor on the device
    text = r.sample_fasta_parts("HG00438.1")    # the same bytes, nothing but metadata decoded on the host
    gz = r.sample_fasta_bgzf("HG00438.1")       # the same text as a BGZF stream (gzip.decompress(gz) == text), compressed on the device
    seqs = r.ranges([("HG00438.1", "chr1", 1000, 1999), (None, "chrM", -1, -1)])   # a list of bytes: letters, one per query
    d, off = r.ranges_dev(queries, letters=False)                                  # symbol codes on the device, query q = d[off[q]:off[q+1]]
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
        self.k, self.min_match_len, self.pack_cardinality = prm["k"], prm["min_match_len"], prm["pack_cardinality"]
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

    def parts(self, name):
        """the sample's stored parts (reader.CAGCFile.GetSampleParts, without the references registered already) -> (the arguments of
        Context.sample_fasta_parts_raw in front of the text buffer, the groups whose references are among the parts)"""
        if self.file is None:
            raise RuntimeError("the reader is closed")
        p = self.file.GetSampleParts(name, self.registered)
        if p is None:
            raise KeyError(name)
        is_ref = p["part_content"] != reader.PART_PACK
        parts = np.zeros(p["part_off"].size, capi.PART_DTYPE)
        parts["off"], parts["n_bytes"], parts["coding"], parts["content"] = p["part_off"], p["part_bytes"], p["part_coding"], p["part_content"]
        parts["gid"] = np.where(is_ref, p["part_group"] + np.uint32(self.gid_base), 0)  # (reader.PART_* and capi.PART_* are the same numbers)
        segs = np.zeros(p["kind"].size, capi.SEG_PART_DTYPE)
        segs["kind"] = p["kind"]
        segs["gid"] = np.where(p["kind"] == capi.SEG_RAW, 0, p["group_id"] + np.uint32(self.gid_base))
        segs["part"], segs["index"], segs["length"], segs["rc"] = p["seg_part"], p["seg_index"], p["length"], p["rc"]
        args = (parts, (p["src"], p["src_bytes"]), self.pack_cardinality, p["ctg_seg"], segs, self.k, self.min_match_len)
        return args, (p["names"], p["name_off"]), p["part_group"][is_ref].tolist()

    def _after(self, rc, new_groups):
        """a call that got as far as the registration has registered every new group, whatever it returned then; one refused before
        that has registered none.  Which it was is asked of the context: a group registers once, so the set must be right."""
        if new_groups and self.ctx.ref_registered(self.gid_base + new_groups[0]):
            self.registered.update(new_groups)
        self.ctx._chk(rc)

    def sample_fasta_parts(self, name, line_length=80):
        """-> bytes: sample_fasta's text; the host decodes nothing but the collection metadata, a refused part raises (no host fallback)"""
        args, (names, name_off), new = self.parts(name)
        rc, need = self.ctx.sample_fasta_parts_raw(*args, line_length, names, name_off, self._pinned, self._pinned_cap)
        if rc == capi.ECAP:  # (the text's size follows from the segments' lengths: nothing was launched or registered)
            rc, need = self.ctx.sample_fasta_parts_raw(*args, line_length, names, name_off, self._pinned_buffer(need), self._pinned_cap)
        self._after(rc, new)
        return C.string_at(self._pinned, need) if need else b""

    def sample_fasta_parts_dev(self, name, line_length=80):
        """-> the same text as a torch uint8 tensor on the context's device"""
        import torch
        args, (names, name_off), new = self.parts(name)
        rc, need = self.ctx.sample_fasta_parts_raw(*args, line_length, names, name_off, None, 0, dev=True)
        if rc != capi.ECAP:
            self._after(rc, new)
        out = torch.empty(need, dtype=torch.uint8, device="cuda")
        if need:
            torch.cuda.synchronize()
            rc, _n = self.ctx.sample_fasta_parts_raw(*args, line_length, names, name_off, out.data_ptr(), need, dev=True)
            self._after(rc, new)
        return out

    def sample_fasta_bgzf(self, name, line_length=80):
        """-> bytes: sample_fasta_parts's text as a BGZF stream (agc_hip_sample_fasta_parts_bgzf) -- multi-member gzip in blocks of 65280
        bytes that gzip.decompress reads and htslib seeks in; the text itself never leaves the device"""
        args, (names, name_off), new = self.parts(name)
        rc, need, _text = self.ctx.sample_fasta_parts_bgzf_raw(*args, line_length, names, name_off, self._pinned, self._pinned_cap)
        if rc == capi.ECAP:  # (the bound follows from the segments' lengths: nothing was launched or registered)
            rc, need, _text = self.ctx.sample_fasta_parts_bgzf_raw(*args, line_length, names, name_off, self._pinned_buffer(need), self._pinned_cap)
        self._after(rc, new)
        return C.string_at(self._pinned, need)

    def sample_fasta_bgzf_dev(self, name, line_length=80):
        """-> (the same stream as a torch uint8 tensor on the context's device, the members' offsets in it: numpy uint64, one per block
        of 65280 text bytes and the EOF member's last)"""
        import torch
        args, (names, name_off), new = self.parts(name)
        rc, need, text = self.ctx.sample_fasta_parts_bgzf_raw(*args, line_length, names, name_off, None, 0, dev=True)
        if rc != capi.ECAP:  # (a stream has 28 bytes at least: anything else is a refusal)
            self._after(rc, new)
        out = torch.empty(need, dtype=torch.uint8, device="cuda")
        off = np.zeros((text + 65279) // 65280 + 1, np.uint64)
        torch.cuda.synchronize()
        rc, n, _text = self.ctx.sample_fasta_parts_bgzf_raw(*args, line_length, names, name_off, out.data_ptr(), need, dev=True, block_off=off)
        self._after(rc, new)
        return out[:n], off

    def range_parts(self, queries):
        """the batch's windows and stored parts (reader.CAGCFile.GetRangeParts, without the references registered already) -> (the
        arguments of Context.ranges_parts_raw in front of `letters`, the groups whose references are among the parts).  An unknown or
        ambiguous contig raises KeyError naming the first such query"""
        if self.file is None:
            raise RuntimeError("the reader is closed")
        p = self.file.GetRangeParts(queries, self.registered)
        if p is None:
            raise RuntimeError("the archive does not hold a part the ranges need")
        is_ref = p["part_content"] != reader.PART_PACK
        parts = np.zeros(p["part_off"].size, capi.PART_DTYPE)
        parts["off"], parts["n_bytes"], parts["coding"], parts["content"] = p["part_off"], p["part_bytes"], p["part_coding"], p["part_content"]
        parts["gid"] = np.where(is_ref, p["part_group"] + np.uint32(self.gid_base), 0)
        wins = np.zeros(p["kind"].size, capi.SEG_WIN_DTYPE)
        wins["kind"] = p["kind"]
        wins["gid"] = np.where(p["kind"] == capi.SEG_RAW, 0, p["group_id"] + np.uint32(self.gid_base))
        wins["part"], wins["index"], wins["length"], wins["rc"] = p["seg_part"], p["seg_index"], p["length"], p["rc"]
        wins["win_from"], wins["win_len"] = p["win_from"], p["win_len"]
        args = (parts, (p["src"], p["src_bytes"]), self.pack_cardinality, p["q_seg"], wins, self.min_match_len)
        return args, p["part_group"][is_ref].tolist()

    def ranges(self, queries, letters=True):
        """queries: a sequence of (sample, contig, start, end), sample may be None -> a list of bytes, one per query: the letters
        GetCtgSeq returns (letters=False: the symbol codes)"""
        args, new = self.range_parts(queries)
        rc, off = self.ctx.ranges_parts_raw(*args, letters, self._pinned, self._pinned_cap)
        if rc == capi.ECAP:  # (the output's size follows from the windows: nothing was launched or registered)
            rc, off = self.ctx.ranges_parts_raw(*args, letters, self._pinned_buffer(int(off[-1])), self._pinned_cap)
        self._after(rc, new)
        data = C.string_at(self._pinned, int(off[-1])) if int(off[-1]) else b""
        return [data[int(off[q]):int(off[q + 1])] for q in range(off.size - 1)]

    def ranges_dev(self, queries, letters=True):
        """-> (the same symbols back to back as a torch uint8 tensor on the context's device, the queries' offsets in it: numpy uint64,
        n_q + 1)"""
        import torch
        args, new = self.range_parts(queries)
        rc, off = self.ctx.ranges_parts_raw(*args, letters, None, 0, dev=True)
        if rc != capi.ECAP:
            self._after(rc, new)
        out = torch.empty(int(off[-1]), dtype=torch.uint8, device="cuda")
        if int(off[-1]):
            torch.cuda.synchronize()
            rc, off = self.ctx.ranges_parts_raw(*args, letters, out.data_ptr(), int(off[-1]), dev=True)
            self._after(rc, new)
        return out, off
