"""A bgzip'd FASTA file's bytes -> its text in HBM and the contigs' byte ranges: what Context.pack_fasta_dev takes.

The stream is inflated on the device (Context.bgzf_inflate_dev: agc_hip_bgzf_inflate_dev, a wavefront per BGZF member); the records
are framed as FastaReader::read_all_mapped frames a plain file (agc_amd/csrc/host/compressor_impl.h): a record starts at byte 0 and at
every '>' that is not inside a header line, its header ends at the first '\\n' or '\\r', framing stops at the first record without name
or without body.  The '>' positions, the line end behind each of them and the header bytes cross to the host; the text does not.

    text, ids, rb, re_ = bgzf_in.fasta_from_bgzf_dev(ctx, open("sample.fa.gz", "rb").read())
    pk, bufs, ctg_off = ctx.pack_fasta_dev(text, text.numel(), rb, re_)
"""
import numpy as np


def fasta_from_bgzf_dev(ctx, data):
    """-> (text: torch uint8 tensor on the device, ids: list of bytes, raw_begin, raw_end: uint64 arrays -- contig c's body, line ends
    included, is text[raw_begin[c]:raw_end[c]])"""
    import torch
    text, _off = ctx.bgzf_inflate_dev(data)
    n = text.numel()
    none = np.zeros(0, np.uint64)
    if n == 0:
        return text, [], none, none
    gt = torch.nonzero(text == ord(">")).flatten()
    le = torch.nonzero((text == 10) | (text == 13)).flatten()
    # a record can start at byte 0 and at a '>': the first line end at or behind each of them (n: none)
    starts = torch.unique(torch.cat([torch.zeros(1, dtype=gt.dtype, device=gt.device), gt]))
    le_n = torch.cat([le, torch.full((1,), n, dtype=le.dtype, device=le.device)])
    ends = le_n[torch.searchsorted(le, starts)].cpu().numpy()
    starts, gt = starts.cpu().numpy(), gt.cpu().numpy()
    recs, s = [], 0
    while s < n:
        e = int(ends[np.searchsorted(starts, s)])
        if e >= n:
            break  # (the header runs into the end of the text)
        j = int(np.searchsorted(gt, e + 1))
        nxt = int(gt[j]) if j < gt.size else n
        if e <= s + 1 or nxt <= e + 1:
            break  # no name or no body
        recs.append((s + 1, e, e + 1, nxt))
        s = nxt
    if not recs:
        return text, [], none, none
    r = np.array(recs, np.int64)
    # the header bytes in one gather
    hl = torch.from_numpy(r[:, 1] - r[:, 0]).to(text.device)
    first = torch.from_numpy(r[:, 0] - np.concatenate([[0], np.cumsum(r[:, 1] - r[:, 0])[:-1]])).to(text.device)
    heads = text[torch.repeat_interleave(first, hl) + torch.arange(int(hl.sum()), device=text.device)].cpu().numpy().tobytes()
    cut = np.concatenate([[0], np.cumsum(r[:, 1] - r[:, 0])])
    ids = [heads[cut[i]:cut[i + 1]] for i in range(len(recs))]
    return text, ids, r[:, 2].astype(np.uint64), r[:, 3].astype(np.uint64)
