"""The life of a device context: what one makes on the GPU it gives back when it is closed."""
import ctypes as C

import numpy as np
import pytest

from agc_amd import synth

pytestmark = pytest.mark.gpu

ARENA_MIN_CHUNK = 256 << 20  # api.hip, arena_next_size: the smallest chunk the reference arena allocates


def _all_kmers(oracle, seq, k):
    out = np.zeros(seq.size, np.uint64)
    n = oracle.lib().agco_enumerate_kmers(seq.ctypes.data_as(C.POINTER(C.c_uint8)), seq.size, k, out.ctypes.data_as(C.POINTER(C.c_uint64)))
    return np.unique(out[:n])


def test_context_lifecycle_returns_its_memory(oracle):
    """Six contexts in a row, each made to create every group of resources a context makes only on demand -- the prefetch, FASTA
    pack and reference-store streams with their events and pinned words, an arena chunk (256 MB at least), both encode lanes'
    scratch, the decode and entropy buffers, the timer pairs, a pinned allocation nobody hands back -- and then closed.  The device
    must have as much free memory after the sixth close as after the first, to within one arena chunk: a chunk leaked per cycle
    alone would cost five of them.  A context made afterwards still scans what the oracle scans."""
    import torch
    from agc_amd import capi
    rng = np.random.default_rng(2024)
    k, mml, gid = 21, 20, 16
    smp = synth.random_seq(rng, 64 << 10)
    off = np.array([0, smp.size], np.uint64)
    ref = synth.mutate(rng, smp[:4096], 0.01)
    spl = _all_kmers(oracle, smp, k)[:1000]
    letters = np.frombuffer(b"ACGT", np.uint8)[smp]
    raw = np.concatenate([np.append(letters[a:a + 60], np.uint8(10)) for a in range(0, letters.size, 60)])
    # (torch's own allocations: made once, so that its caching allocator asks the device for nothing between the measurements)
    d_codes = torch.from_numpy(smp).cuda()
    d_raw = torch.from_numpy(np.concatenate([raw, np.zeros(64, np.uint8)])).cuda()
    torch.cuda.synchronize()
    want_z = None
    free = []
    for cycle in range(6):
        ctx = capi.Context(0)
        ctx.timing(True)
        ctx.splitters_set(spl)
        pk, keep = ctx.pack_dev(d_codes)
        ctx.prefetch_packed_dev(pk, off, k)
        hits = ctx.scan_prefetched(pk, off, k)
        assert hits[1].size > 0
        pk2, keep2, off2 = ctx.pack_fasta_end(ctx.pack_fasta_begin(d_raw, raw.size, [0], [raw.size]))
        assert int(off2[-1]) == smp.size
        ctx.ref_register(gid, ref, mml)
        for lane in (0, 1):
            ctx.lz_encode_begin_packed(pk, [gid], [0], [4096], lane=lane)
        enc, eoff = ctx.lz_encode_end_on(0)
        enc1, _ = ctx.lz_encode_end_on(1)
        assert np.array_equal(enc, enc1) and np.array_equal(enc, oracle.LZ(ref, mml).encode(smp[:4096]))
        ctx.ref_store_begin_packed(0, 1, pk, [0], [4096])
        _cnt, _cur, out, _ooff = ctx.ref_store_end(0)
        assert np.array_equal(out, smp[:4096])
        dec, _ = ctx.lz_decode_batch(enc, eoff, [gid])
        assert np.array_equal(dec, smp[:4096])
        z = ctx.zstd17_batch([raw[:1024].tobytes()])
        want_z = want_z or z
        assert z == want_z and len(z[0]) > 0
        assert ctx.host_alloc(4096)  # (deliberately not handed back)
        assert ctx.timing_get()["scan"][1] >= 1
        ctx.close()
        del pk, keep, pk2, keep2
        torch.cuda.synchronize()
        free.append(torch.cuda.mem_get_info()[0])
    print("free bytes after each close:", free)
    assert free[5] > free[0] - ARENA_MIN_CHUNK, free
    # a context made after all that works
    spl2 = oracle.determine_splitters([smp], k, 1000)
    ctx = capi.Context(0)
    ctx.splitters_set(spl2)
    _c, pos, hd, hr = ctx.scan_contigs(smp, off, k)
    ctx.close()
    s = oracle.scan_contig(smp, k, spl2)
    m = s["back_full"] == 1
    assert m.sum() > 20
    assert np.array_equal(pos, s["start"][m] + s["len"][m] - 1) and np.array_equal(hd, s["back_dir"][m]) and np.array_equal(hr, s["back_rc"][m])
