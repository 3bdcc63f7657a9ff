"""GPU parity: the device segment table (seg_kernels.hip, segments.hip) at its table, contig and group edges.

agc_hip_segments_packed against the oracle's compress_contig per contig and a Python dictionary of the group table, at the shapes
the host depends on and the other files do not reach: a table of several LDS ranges with probe chains that leave their range, wrap
around the table's end and pass keys equal in one half only; thousands of contigs of every edge shape; the three reasons a known
group is not encoded; table updates of several blocks back to back; and the return codes of every refusal."""
import ctypes as C

import numpy as np
import pytest

from agc_amd import capi, synth

pytestmark = pytest.mark.gpu

RANGE = 4096  # slots a block of group_lookup_kernel stages in LDS (seg_kernels.hip: GM_RANGE_SLOTS)
M64 = (1 << 64) - 1
FIELDS = ("ctg", "start", "len", "front_full", "back_full", "front_dir", "front_rc", "back_dir", "back_rc", "store_rc", "map_gid")


def group_hash(k1, k2):
    """agc_hip_group_hash (seg_kernels.hip: group_hash) in Python integers, to lay tables out with"""
    h = (k1 * 0x9E3779B97F4A7C15) & M64
    h ^= (h >> 32) ^ ((k2 * 0xC2B2AE3D27D4EB4F) & M64)
    return h ^ (h >> 29)


# ---- what the oracle cuts ---------------------------------------------------------------------------------------------------
def oracle_segments(oracle, contigs, k, spl):
    """compress_contig per contig -> (the segments as the device reports them, map_gid still -1; per segment its key or None)"""
    parts = []
    for ci, c in enumerate(contigs):
        s = oracle.scan_contig(c, k, spl)
        n = len(s["start"])
        if not n:
            continue
        a = np.zeros(n, capi.SEGMENT_DTYPE)
        a["ctg"], a["start"], a["len"] = ci, s["start"], s["len"]
        for side in ("front", "back"):
            full = s[side + "_full"] != 0
            a[side + "_full"] = full
            a[side + "_dir"] = np.where(full, s[side + "_dir"], 0)
            a[side + "_rc"] = np.where(full, s[side + "_rc"], 0)
        parts.append(a)
    w = np.concatenate(parts) if parts else np.zeros(0, capi.SEGMENT_DTYPE)
    both = (w["front_full"] != 0) & (w["back_full"] != 0)
    f, b = np.minimum(w["front_dir"], w["front_rc"]), np.minimum(w["back_dir"], w["back_rc"])
    # the key (min, max) of the two canonical k-mers and its orientation (add_segment)
    w["store_rc"] = both & ~(f < b)
    w["map_gid"] = -1
    k1, k2 = np.where(f < b, f, b).tolist(), np.where(f < b, b, f).tolist()
    keys = [(k1[i], k2[i]) if both[i] else None for i in range(w.size)]
    return w, keys


def with_gids(want, keys, table):
    w = want.copy()
    w["map_gid"] = [table.get(q, -1) if q is not None else -1 for q in keys]
    return w


def assert_segments(got, want, what, fields=FIELDS):
    assert len(got) == len(want), f"{what}: {len(got)} segments, the oracle cuts {len(want)}"
    for f in fields:
        if not np.array_equal(got[f], want[f]):
            i = int(np.argmax(got[f] != want[f]))
            raise AssertionError(f"{what}: segment {i} of {len(want)}, field {f}: got {got[i]} want {want[i]}")


_CASES = {}


def sample_case(oracle, k, seed):
    """a random reference of 400 000 symbols, its splitters at segment size 200, one mutated sample: about 1900 segments"""
    if (k, seed) not in _CASES:
        rng = np.random.default_rng(seed)
        ref = synth.random_seq(rng, 400_000)
        spl = oracle.determine_splitters([ref], k, 200)
        smp = synth.mutate(rng, ref, 0.002)
        want, keys = oracle_segments(oracle, [smp], k, spl)
        distinct = list(dict.fromkeys(q for q in keys if q is not None))
        _CASES[(k, seed)] = dict(k=k, spl=spl, smp=smp, want=want, keys=keys, distinct=distinct)
    return _CASES[(k, seed)]


def pack(ctx, codes):
    import torch
    d = torch.from_numpy(np.ascontiguousarray(codes)).cuda()
    torch.cuda.synchronize()
    pk, keep = ctx.pack_dev(d)
    return pk, (keep, d)


def offsets(contigs):
    off = np.zeros(len(contigs) + 1, np.uint64)
    off[1:] = np.cumsum([c.size for c in contigs])
    return off


def raw_segments(ctx, pk, off, k, cap, prefetched=0, encode_known=0):
    """agc_hip_segments_packed as it is -> (return code, *h_n_segs, *h_n_encoded, the buffer)"""
    off = np.ascontiguousarray(off, np.uint64)
    buf = np.zeros(cap, capi.SEGMENT_DTYPE) if cap else None
    n, ne = C.c_uint64(), C.c_uint32()
    rc = ctx.L.agc_hip_segments_packed(ctx.h, C.byref(pk), capi._p(off, capi.u64p), off.size - 1, k, prefetched, encode_known, cap,
                                       buf.ctypes.data if cap else None, C.byref(n), C.byref(ne))
    return rc, int(n.value), int(ne.value), buf


def upper_bound(ctx, pk, off, k):
    """n_ub = raw hits + contigs, as a call without room learns it"""
    rc, n_ub, _ne, _buf = raw_segments(ctx, pk, off, k, 0)
    assert rc == capi.ECAP
    return n_ub


# ---- tables with chosen chains ----------------------------------------------------------------------------------------------
def lay_out(n_slots, runs, keys_to_gid):
    """runs: [(first index, [(k1, k2, gid), ...])], written first, slot after slot (modulo n_slots), wherever they are told to sit;
    then the real keys by linear probing from their home slots.  At least half of the slots stay free: a chain without a free slot
    would never end on the device."""
    assert n_slots >= 16 and n_slots & (n_slots - 1) == 0
    tab = np.zeros(n_slots, capi.GROUP_SLOT_DTYPE)
    for first, slots in runs:
        for j, (k1, k2, gid) in enumerate(slots):
            tab[(first + j) & (n_slots - 1)] = (k1, k2, gid, 1)
    for (k1, k2), gid in keys_to_gid.items():
        i = group_hash(k1, k2) & (n_slots - 1)
        while tab[i]["used"]:
            assert (int(tab[i]["k1"]), int(tab[i]["k2"])) != (k1, k2)
            i = (i + 1) & (n_slots - 1)
        tab[i] = (k1, k2, gid, 1)
    assert int((tab["used"] == 0).sum()) * 2 >= n_slots, "a table for the device keeps half of its slots free"
    return tab


def probe(tab, key):
    """the look-up on the numpy copy -> (gid or -1, the slots the chain visits, the last one being the match or the free slot)"""
    mask = tab.size - 1
    i = group_hash(*key) & mask
    path = []
    while True:
        path.append(i)
        assert len(path) <= tab.size
        g = tab[i]
        if not g["used"]:
            return -1, path
        if (int(g["k1"]), int(g["k2"])) == key:
            return int(g["gid"]), path
        i = (i + 1) & mask


_TABLES = {}


def adversarial_table(case, n_slots):
    """the sample's keys in a table of n_slots whose chains leave their LDS range, wrap and pass near misses -> (table, {key: gid},
    what was arranged); every arrangement is asserted on the numpy copy here, before any table reaches the device"""
    if (case["k"], n_slots) in _TABLES:
        tab, table, info = _TABLES[(case["k"], n_slots)]
        return tab.copy(), dict(table), info
    distinct, mask = case["distinct"], n_slots - 1
    keyset = set(distinct)
    home = {q: group_hash(*q) & mask for q in distinct}
    last = n_slots // RANGE - 1
    assert last >= 1
    # nearest below a range end first (not the last range: its end is the table's, which the wrapped key has for itself)
    near_end = sorted((q for q in distinct if home[q] // RANGE != last and q[0] != q[1]), key=lambda q: RANGE - 1 - home[q] % RANGE)
    lost, crossing = near_end[0], near_end[1:5]
    wrapped = max((q for q in distinct if q[0] != q[1]), key=home.get)
    assert home[wrapped] // RANGE == last and wrapped not in crossing and wrapped != lost
    middle = []
    for q in distinct:
        if 1000 <= home[q] % RANGE < 3000 and q[0] != q[1] and all(abs(home[q] - home[p]) >= 16 for p in middle):
            middle.append(q)
        if len(middle) == 4:
            break
    special = set(crossing) | {wrapped} | set(middle)
    left_out = (set(distinct[::5]) - special) | {lost}
    table = {q: g for g, q in enumerate(q for q in distinct if q not in left_out)}  # gids from 0: some below 16
    assert min(table.values()) == 0 and len(left_out) >= 310
    n_decoys = [0]

    def decoys(n):  # odd k-mers: a left-aligned k-mer of k < 32 symbols ends in zero bits
        out = []
        for _ in range(n):
            n_decoys[0] += 1
            out.append((2 * n_decoys[0] + 1, (1 << 63) | (2 * n_decoys[0] + 1), 500_000 + n_decoys[0]))
        return out

    def near_misses(q):  # equal to q in one half only, and q's halves swapped: each with a gid of its own
        n_decoys[0] += 3
        return [(q[0], q[1] ^ 4, 600_000 + n_decoys[0]), (q[0] ^ 4, q[1], 600_001 + n_decoys[0]), (q[1], q[0], 600_002 + n_decoys[0])]

    runs = []
    for q in crossing + [lost]:  # from the home slot up to and two slots past the end of its range
        end = (home[q] // RANGE + 1) * RANGE
        runs.append((home[q], decoys(end + 2 - home[q])))
    runs.append((home[wrapped], decoys(n_slots - home[wrapped]) + near_misses(wrapped)))  # ... to the last slot, near misses in slots 0-2
    for q in middle:
        runs.append((home[q], near_misses(q)))
    for _first, slots in runs:
        assert all((k1, k2) not in keyset for (k1, k2, _g) in slots), "a decoy occurs nowhere in the sample"
    tab = lay_out(n_slots, runs, table)
    # ---- what the table must hold, on the numpy copy
    n_cross = n_wrap = n_near = 0
    for q in distinct:
        gid, path = probe(tab, q)
        assert gid == table.get(q, -1), q
        if q in table:
            n_wrap += path[-1] < path[0]
            n_cross += path[-1] > path[0] and path[-1] // RANGE != path[0] // RANGE
            before = [(int(tab[i]["k1"]), int(tab[i]["k2"])) for i in path[:-1]]
            n_near += (any(a == q[0] and b != q[1] for a, b in before) and any(a != q[0] and b == q[1] for a, b in before) and (q[1], q[0]) in before)
    assert n_cross >= 3 and n_wrap >= 1 and n_near >= 3, (n_cross, n_wrap, n_near)
    gid, path = probe(tab, lost)  # a key the table does not hold: through a decoy run to a free slot of the next range
    assert gid == -1 and len(path) > 2 and path[-1] // RANGE == path[0] // RANGE + 1 and not tab[path[-1]]["used"]
    info = dict(left_out=[q for q in distinct if q in left_out], lost=lost, crossing=crossing, wrapped=wrapped)
    _TABLES[(case["k"], n_slots)] = (tab, table, info)
    return tab.copy(), dict(table), info


def staged_sample(case):
    """the 400 kbp sample as one contig and 400 contigs of 5 symbols behind it: enough segments for the staged look-up"""
    rng = np.random.default_rng(5)
    contigs = [case["smp"]] + [synth.random_seq(rng, 5) for _ in range(400)]
    return contigs, offsets(contigs)


def check_windows(hip_ctx, oracle, case, pk, n_slots, table, what):
    """the same table, batches too small for staging: windows of 20 kbp of the main contig, one per call"""
    k, smp = case["k"], case["smp"]
    for a in range(0, smp.size, 20_000):
        off = np.array([a, min(a + 20_000, smp.size)], np.uint64)
        n_ub = upper_bound(hip_ctx, pk, off, k)
        assert n_ub * 8 < n_slots  # segments.hip: `staged` needs n_ub * 8 >= n_slots, so this call reads the table from HBM
        want, keys = oracle_segments(oracle, [smp[int(off[0]):int(off[1])]], k, case["spl"])
        segs, _ = hip_ctx.segments_packed(pk, off, k, cap=n_ub)
        assert_segments(segs, with_gids(want, keys, table), f"{what}, window at {a}")


# ---- 1. look-up across ranges -----------------------------------------------------------------------------------------------
def test_group_hash_in_python_is_the_library_s():
    L = capi.load()
    rng = np.random.default_rng(1)
    for k1, k2 in [(0, 0), (1, 0), (0, 1), (M64, M64), (1 << 63, 1 << 22)] + [tuple(int(x) for x in rng.integers(0, 1 << 63, 2)) for _ in range(20)]:
        assert int(L.agc_hip_group_hash(k1, k2)) == group_hash(k1, k2)


@pytest.mark.parametrize("k,n_slots", [(21, 8192), (31, 16384)])
def test_lookup_across_lds_ranges(hip_ctx, oracle, k, n_slots):
    """group_lookup_kernel with several staged ranges: chains that leave their block's range (HBM behind LDS), a chain that wraps
    from the last slot to slot 0, near-miss keys in front of the real one, keys the table does not hold -- and the same chains
    straight from HBM"""
    case = sample_case(oracle, k, 1)
    tab, table, info = adversarial_table(case, n_slots)
    contigs, off = staged_sample(case)
    want, keys = oracle_segments(oracle, contigs, k, case["spl"])
    want = with_gids(want, keys, table)
    left_out = set(info["left_out"])
    assert sum(q in left_out for q in keys) >= 300 and info["lost"] in keys
    pk, keep = pack(hip_ctx, np.concatenate(contigs))
    hip_ctx.splitters_set(case["spl"])
    hip_ctx.group_map_upload(tab)
    n_ub = upper_bound(hip_ctx, pk, off, k)
    assert n_ub * 8 >= n_slots >= 2 * RANGE  # segments.hip: `staged` = n_ub * 8 >= n_slots; two ranges or more
    segs, _ = hip_ctx.segments_packed(pk, off, k, cap=n_ub)
    assert_segments(segs, want, "staged")
    check_windows(hip_ctx, oracle, case, pk, n_slots, table, "from HBM")


# ---- 2. contigs -------------------------------------------------------------------------------------------------------------
SHAPES = ("slice", "empty", "one", "k-1", "k", "splitter", "ends on a hit", "begins with a splitter", "N only")


def contig_zoo(case):
    rng = np.random.default_rng(77)
    k, smp, want = case["k"], case["smp"], case["want"]
    ends = (want["start"] + want["len"] - 1)[want["back_full"] != 0].astype(np.int64)  # last symbols of the taken hits
    ends = ends[(ends > 4000) & (ends < smp.size - 4000)]
    contigs, shape = [], []
    for i in range(9 * 280):
        s = SHAPES[i % 9]
        n = int(rng.integers(300, 3001))
        p = int(ends[rng.integers(0, ends.size)])
        a = int(rng.integers(0, smp.size - n))
        c = {"slice": smp[a:a + (n | 1)], "empty": smp[:0], "one": smp[a:a + 1], "k-1": smp[a:a + k - 1], "k": smp[a:a + k],
             "splitter": smp[p + 1 - k:p + 1], "ends on a hit": smp[p + 1 - n:p + 1], "begins with a splitter": smp[p + 1 - k:p + 1 - k + n],
             "N only": np.full(1 + n % 50, 4, np.uint8)}[s]
        contigs.append(c.copy())
        shape.append(i % 9)
    for i in (1500, 1501, len(contigs), len(contigs) + 1):  # empty contigs side by side, and at the sample's end
        contigs[i:i + 1] = [smp[:0].copy()]
        shape[i:i + 1] = [SHAPES.index("empty")]
    return contigs, np.array(shape)


def test_thousands_of_contigs_of_every_edge_shape(hip_ctx, oracle):
    """2522 contigs -- three trips of contig_sums_kernel's block-wide scan and its carry --, among them empty ones, contigs of
    1, k - 1 and k symbols, a contig that is one splitter, contigs that end on a hit or begin with a splitter, contigs of N: the
    oracle's segments; again from a sample that starts at an odd offset; again with the scan prefetched"""
    k = 21
    case = sample_case(oracle, k, 1)
    contigs, shape = contig_zoo(case)
    off = offsets(contigs)
    assert len(contigs) >= 2500
    for s in range(9):  # every shape on both sides of the scan's trips
        at = np.flatnonzero(shape == s)
        assert (at < 1024).any() and ((at >= 1024) & (at < 2048)).any() and (at >= 2048).any(), SHAPES[s]
    want, keys = oracle_segments(oracle, contigs, k, case["spl"])
    per = np.bincount(want["ctg"], minlength=len(contigs))
    assert not per[shape == SHAPES.index("empty")].any()
    assert (per[shape == SHAPES.index("splitter")] == 2).all() and (want["len"][np.isin(want["ctg"], np.flatnonzero(shape == SHAPES.index("splitter")))] == k).all()
    table = {q: g for g, q in enumerate(q for q in dict.fromkeys(keys) if q is not None) if g % 3}
    assert len(table) > 500
    assert int(off[1]) % 2 == 1 and per[0] > 0  # (for the second call: an odd first offset, and contig indices that shift)
    pk, keep = pack(hip_ctx, np.concatenate(contigs))
    hip_ctx.splitters_set(case["spl"])
    hip_ctx.group_map_set(table)
    segs, _ = hip_ctx.segments_packed(pk, off, k, cap=16)
    assert_segments(segs, with_gids(want, keys, table), "2522 contigs")
    # the same without the first contig: h_ctg_off[0] != 0
    rest = want["ctg"] > 0
    want1 = with_gids(want, keys, table)[rest]
    want1["ctg"] -= 1
    segs, _ = hip_ctx.segments_packed(pk, off[1:], k, cap=16)
    assert_segments(segs, want1, "from the second contig on")
    for o, w, what in ((off, with_gids(want, keys, table), "prefetched"), (off[1:], want1, "prefetched, from the second contig on")):
        hip_ctx.prefetch_packed_dev(pk, o, k)
        segs, _ = hip_ctx.segments_packed(pk, o, k, prefetched=True, cap=16)
        assert_segments(segs, w, what)


# ---- 3. who is encoded ------------------------------------------------------------------------------------------------------
MML = 20


def known_groups(oracle, case, n_known):
    """references for the first n_known keys at the even gids from 16 on, three more classes of keys the table knows and the encode
    must leave alone -> ({key: gid}, {key: reference} of the first class, {gid: reference} to register)"""
    rng = np.random.default_rng(33)
    smp, want, keys, distinct = case["smp"], case["want"], case["keys"], case["distinct"]
    assert len(distinct) >= n_known + 24 and n_known >= 8

    def reference(q):  # the first segment of the key, as the key orients it, slightly edited
        i = keys.index(q)
        t = smp[int(want["start"][i]):int(want["start"][i]) + int(want["len"][i])]
        return synth.mutate(rng, oracle.rev_comp(t) if want["store_rc"][i] else t, 0.003)

    table, refs, register = {}, {}, {}
    for j, q in enumerate(distinct[:n_known]):
        table[q] = 16 + 2 * j
        refs[q] = register[table[q]] = reference(q)
    top = 16 + 2 * (n_known - 1)  # the highest registered gid: n_refs = top + 1
    low = distinct[n_known:n_known + 8]
    for j, q in enumerate(low):  # gids 3 to 10: below 16; 3 and 4 with a reference of their own
        table[q] = 3 + j
        if j < 2:
            register[3 + j] = reference(q)
    odd = list(range(17, top, 2))
    holes = sorted(set(odd[::max(1, len(odd) // 8)][:7] + [odd[-1]]))
    assert len(holes) >= 7 and all(g % 2 == 1 and 16 < g < top for g in holes)
    for q, g in zip(distinct[n_known + 8:n_known + 16], holes):  # inside the registered span, never registered
        table[q] = g
    for q, g in zip(distinct[n_known + 16:n_known + 24], [top + 1, top + 2, 1000 + top, 60_000, 100_000, 1 << 20, 1 << 30, (1 << 31) - 1]):
        table[q] = g  # at and above n_refs
    assert sorted(register) == [3, 4] + list(range(16, top + 1, 2))
    return table, refs, register


def expected_deltas(oracle, case, refs, off0=0, want=None, keys=None):
    """the deltas of the segments whose key has a reference, in segment order"""
    want, keys = (case["want"], case["keys"]) if want is None else (want, keys)
    lz = {q: oracle.LZ(r, MML) for q, r in refs.items()}
    out = []
    for i, q in enumerate(keys):
        if q in refs:
            a = off0 + int(want["start"][i])
            t = case["smp"][a:a + int(want["len"][i])]
            out.append(lz[q].encode(oracle.rev_comp(t) if want["store_rc"][i] else t))
    return out


def assert_deltas(enc, eoff, deltas, what):
    assert eoff.size == len(deltas) + 1, f"{what}: {eoff.size - 1} deltas, expected {len(deltas)}"
    for i, d in enumerate(deltas):
        assert np.array_equal(enc[int(eoff[i]):int(eoff[i + 1])], d), f"{what}: delta {i}"


def test_only_registered_groups_from_16_on_are_encoded(oracle):
    """known_flag_kernel: a segment is encoded when the table knows its key AND the gid is at least 16, below the number of
    reference descriptors, and has a reference.  64 such keys beside 8 with gids 3-10 (two of them registered), 8 in never-registered
    holes of the registered span and 8 at and far above its end"""
    k = 21
    case = sample_case(oracle, k, 1)
    smp = case["smp"]
    off = np.array([0, smp.size], np.uint64)
    table, refs, registered = known_groups(oracle, case, 64)
    want = with_gids(case["want"], case["keys"], table)
    encoded = np.array([q in refs for q in case["keys"]])
    deltas = expected_deltas(oracle, case, refs)
    per_key = {q: case["keys"].count(q) for q in refs}
    assert len(per_key) == 64 and len(deltas) == sum(per_key.values()) == int(encoded.sum())
    gids = sorted(set(table.values()) - set(registered))  # the other three classes: 6 below 16, 8 holes, 8 from n_refs on
    assert len(gids) == 22 and gids[5] == 10 and gids[6] == 17 and gids[13] == 141 and gids[14] == 143 and set(gids) <= set(want["map_gid"].tolist())
    ctx = capi.Context(0)  # (a fresh one: the number of its reference descriptors is this test's)
    try:
        for gid, ref in registered.items():
            ctx.ref_register(gid, ref, MML)
        pk, keep = pack(ctx, smp)
        ctx.splitters_set(case["spl"])
        ctx.group_map_set(table)
        segs, n_enc = ctx.segments_packed(pk, off, k, encode_known=True, cap=16)
        assert_segments(segs, want, "encode_known = 1")
        assert np.array_equal(segs["encoded"] != 0, encoded), np.flatnonzero((segs["encoded"] != 0) != encoded)[:8]
        assert n_enc == len(deltas)
        enc, eoff = ctx.lz_encode_end()
        assert_deltas(enc, eoff, deltas, "encode_known = 1")
        # the launch as a call of its own
        segs, n_enc = ctx.segments_packed(pk, off, k, cap=1 << 12)
        assert_segments(segs, want, "encode_known = 0")
        assert n_enc == 0 and not segs["encoded"].any()
        m = ctx.segments_encode_known(segs, registered)
        assert np.array_equal(m, encoded)
        enc2, eoff2 = ctx.lz_encode_end()
        assert np.array_equal(enc2, enc) and np.array_equal(eoff2, eoff)
        # a table that knows nothing: nothing is encoded and nothing stays in flight
        ctx.group_map_set({})
        segs, n_enc = ctx.segments_packed(pk, off, k, encode_known=True, cap=1 << 12)
        assert_segments(segs, with_gids(case["want"], case["keys"], {}), "empty table")
        assert n_enc == 0 and not segs["encoded"].any()
        n = C.c_uint32(99)
        assert ctx.L.agc_hip_lz_encode_pending(ctx.h, C.byref(n)) == capi.OK and n.value == 0
        assert ctx.L.agc_hip_segments_encode_known(ctx.h) == capi.EINVAL  # (that call had its launch)
    finally:
        ctx.close()


# ---- 4. table updates -------------------------------------------------------------------------------------------------------
def test_table_updates_of_several_blocks_back_to_back(hip_ctx, oracle):
    """agc_hip_group_map_update: 600 slots in one call (three blocks of gmap_scatter_kernel) -- 300 keys move to other groups, 300
    keys the table did not hold arrive at the free slots that end their chains --, a second update right behind it (the staging
    buffer is reused behind the first one's event), then the look-up: every map_gid follows the numpy copy"""
    k, n_slots = 21, 8192
    case = sample_case(oracle, k, 1)
    tab, table, info = adversarial_table(case, n_slots)
    contigs, off = staged_sample(case)
    want, keys = oracle_segments(oracle, contigs, k, case["spl"])
    tab0 = tab.copy()

    def move(q, gid):
        g, path = probe(tab, q)
        assert g == table[q]
        tab[path[-1]]["gid"] = table[q] = gid
        return path[-1]

    def arrive(q, gid):
        g, path = probe(tab, q)
        assert g == -1 and q not in table
        tab[path[-1]] = (q[0], q[1], gid, 1)
        table[q] = gid
        return path[-1]

    present = info["crossing"] + [info["wrapped"]] + [q for q in table if q not in info["crossing"] and q != info["wrapped"]][:295]
    absent = [info["lost"]] + [q for q in info["left_out"] if q != info["lost"]]
    assert len(present) == 300 and len(absent) >= 303
    idx1 = [move(q, table[q] + 100_000) for q in present] + [arrive(q, 200_000 + j) for j, q in enumerate(absent[:300])]
    slots1 = tab[idx1].copy()
    # the second update: three of the keys that just moved move again, two more arrive
    idx2 = [move(q, 400_000 + j) for j, q in enumerate(present[:3])] + [arrive(q, 300_000 + j) for j, q in enumerate(absent[300:302])]
    slots2 = tab[idx2].copy()
    assert len(set(idx1)) == len(idx1) == 600 and len(set(idx2)) == 5 and int((tab["used"] == 0).sum()) * 2 >= n_slots
    for q in case["distinct"]:
        assert probe(tab, q)[0] == table.get(q, -1)
    pk, keep = pack(hip_ctx, np.concatenate(contigs))
    hip_ctx.splitters_set(case["spl"])
    hip_ctx.group_map_upload(tab0)
    hip_ctx.group_map_update(idx1, slots1)
    hip_ctx.group_map_update(idx2, slots2)
    n_ub = upper_bound(hip_ctx, pk, off, k)
    assert n_ub * 8 >= n_slots  # segments.hip: the staged look-up
    segs, _ = hip_ctx.segments_packed(pk, off, k, cap=n_ub)
    assert_segments(segs, with_gids(want, keys, table), "after two updates")
    got = segs["map_gid"].tolist()
    assert sum(200_000 <= g < 200_300 for g in got) >= 300 and sum(300_000 <= g < 300_002 for g in got) >= 2 and sum(g >= 400_000 for g in got) >= 3


# ---- 5. contracts -----------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_context_working(oracle):
    """the return codes of agc_hip_segments_packed, agc_hip_segments_encode_known and agc_hip_group_map_*; after every refusal an
    ordinary agc_hip_segments_packed on the same context gives the oracle's segments and the table's groups"""
    k = 21
    case = sample_case(oracle, k, 1)
    smp = case["smp"][:60_000]
    off = np.array([0, smp.size], np.uint64)
    win = np.array([1, 20_000], np.uint64)
    want, keys = oracle_segments(oracle, [smp], k, case["spl"])
    wwin, kwin = oracle_segments(oracle, [smp[int(win[0]):int(win[1])]], k, case["spl"])
    ctx = capi.Context(0)
    try:
        L, h = ctx.L, ctx.h
        slot = np.zeros(1, capi.GROUP_SLOT_DTYPE)
        idx = np.zeros(1, np.uint64)
        assert L.agc_hip_segments_encode_known(h) == capi.EINVAL  # nothing on the device yet
        assert L.agc_hip_group_map_update(h, 1, capi._p(idx, capi.u64p), slot.ctypes.data) == capi.EINVAL  # no table set
        table, refs, registered = known_groups(oracle, case, 8)
        deltas = expected_deltas(oracle, case, refs, 0, want, keys)
        assert len(deltas) >= 8
        for gid, ref in registered.items():
            ctx.ref_register(gid, ref, MML)
        pk, keep = pack(ctx, smp)
        ctx.splitters_set(case["spl"])
        tab = ctx.group_map_set(table)

        def still_works(what):
            segs, _ = ctx.segments_packed(pk, win, k, cap=16)
            assert_segments(segs, with_gids(wwin, kwin, table), "after " + what)

        still_works("the first two refusals")
        for bad_k in (15, 33):
            assert raw_segments(ctx, pk, off, bad_k, 1 << 12)[0] == capi.EINVAL
            still_works(f"k = {bad_k}")
        assert raw_segments(ctx, pk, np.array([0, smp.size + 1], np.uint64), k, 1 << 12)[0] == capi.EINVAL
        still_works("contigs beyond the sample")
        assert raw_segments(ctx, pk, off[:1], k, 1 << 12)[:3] == (capi.OK, 0, 0)
        still_works("no contigs")
        for bad_n in (24, 8):
            assert L.agc_hip_group_map_set(h, tab.ctypes.data, bad_n) == capi.EINVAL
            still_works(f"a table of {bad_n} slots")
        idx[0] = tab.size
        assert L.agc_hip_group_map_update(h, 1, capi._p(idx, capi.u64p), slot.ctypes.data) == capi.EINVAL
        still_works("an update beyond the table")
        # an encode in flight: no second one, no launch of its own; the one in flight arrives whole
        segs, n_enc = ctx.segments_packed(pk, off, k, encode_known=True, cap=1 << 12)
        assert n_enc == len(deltas)
        assert L.agc_hip_segments_encode_known(h) == capi.EINVAL
        assert raw_segments(ctx, pk, off, k, 1 << 12, encode_known=1)[0] == capi.EINVAL
        enc, eoff = ctx.lz_encode_end()
        assert_deltas(enc, eoff, deltas, "after a refused second encode")
        still_works("a refused second encode")
        # ... and once it was collected, its segments are not encoded a second time
        segs, n_enc = ctx.segments_packed(pk, off, k, encode_known=True, cap=1 << 12)
        enc, eoff = ctx.lz_encode_end()
        assert_deltas(enc, eoff, deltas, "encode_known = 1")
        assert L.agc_hip_segments_encode_known(h) == capi.EINVAL
        n = C.c_uint32(99)
        assert L.agc_hip_lz_encode_pending(h, C.byref(n)) == capi.OK and n.value == 0
        still_works("a launch behind encode_known = 1")
        # the launch as a call of its own, once
        segs, _ = ctx.segments_packed(pk, off, k, cap=1 << 12)
        ctx.segments_encode_known(segs, registered)
        assert L.agc_hip_segments_encode_known(h) == capi.EINVAL
        enc, eoff = ctx.lz_encode_end()
        assert_deltas(enc, eoff, deltas, "after a refused second launch")
        still_works("a second launch")
    finally:
        ctx.close()
