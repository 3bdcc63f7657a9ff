"""Hand-laid sample plans for the FASTA text kernels (tests/test_fasta_out_host.py runs fasta_out.h's chunk walk over them on the
CPU, tests/test_gpu_fasta_out.py the whole call on the device) and the text they must give, built here in numpy from the
contigs' symbols -- nothing of the kernel's arithmetic is used.

A case: {"name", "k", "line_length", "refs": [symbols of a group reference, ...], "contigs": [(name bytes, [segment, ...]), ...]}
A segment: {"kind": RAW / REF / DELTA, "rc", "stored": its symbols as the archive stores them (before rc), "ref": index into refs}
(REF: stored is refs[ref]; DELTA: stored is what its delta against refs[ref] decodes to).  The overlap symbols in front of a
segment that is not its contig's first are NOT the tail of the segment before (in an archive they are): a wrong skip shows."""
import numpy as np

from agc_amd import capi, synth

RAW, REF, DELTA = 0, 1, 2
MML = 20
ALPHA = np.frombuffer(b"ACGTNRYSWKMBDHVU" + b" " * 240, np.uint8)
NAME_LENGTHS = (1, 14, 15, 16, 17, 300)
LINE_LENGTHS = (1, 3, 15, 16, 17, 60, 80, 0, 5000)  # (5000: larger than every contig of the grid)


def rev_comp(s):
    r = s[::-1].copy()
    m = r < 4
    r[m] = 3 - r[m]
    return r


def seg(kind, stored, rc=0, ref=None):
    return {"kind": kind, "rc": int(rc), "stored": np.ascontiguousarray(stored, np.uint8), "ref": ref}


def oriented(s):
    return rev_comp(s["stored"]) if s["rc"] else s["stored"]


def kept(segs, k):
    """symbols every segment of a contig contributes"""
    return [oriented(s)[0 if i == 0 else k:] for i, s in enumerate(segs)]


def contig_symbols(segs, k):
    return np.concatenate(kept(segs, k) + [np.zeros(0, np.uint8)])


def contig_text(name, sym, line_length):
    L = line_length or sym.size
    a = ALPHA[sym]
    out = [b">" + name + b"\n"]
    full = sym.size // L * L if sym.size else 0
    if full:
        b = np.empty((full // L, L + 1), np.uint8)
        b[:, :L] = a[:full].reshape(-1, L)
        b[:, L] = 10
        out.append(b.tobytes())
    if sym.size > full:
        out.append(a[full:].tobytes() + b"\n")
    return b"".join(out)


def expected_text(case):
    return b"".join(contig_text(n, contig_symbols(s, case["k"]), case["line_length"]) for n, s in case["contigs"])


def contig_text_size(name_len, n_sym, line_length):
    L = line_length or n_sym
    return name_len + 2 + (n_sym + (n_sym + L - 1) // L if n_sym else 0)


def plan_arrays(case, gid0, oracle):
    """the case as agc_hip_sample_fasta takes it (the arguments of capi.Context.sample_fasta): reference i is group gid0 + i, the
    deltas are the oracle's"""
    lz = {}
    segs, blob, ctg_seg, names, name_off, n_blob = [], [], [0], [], [0], 0
    for name, ss in case["contigs"]:
        for s in ss:
            b = np.zeros(0, np.uint8)
            if s["kind"] == RAW:
                b = s["stored"]
            elif s["kind"] == DELTA:
                if s["ref"] not in lz:
                    lz[s["ref"]] = oracle.LZ(case["refs"][s["ref"]], MML)
                b = lz[s["ref"]].encode(s["stored"])
                assert b.size or not s["stored"].size
            segs.append((s["kind"], 0 if s["kind"] == RAW else gid0 + s["ref"], n_blob, b.size, s["stored"].size, s["rc"], 0))
            blob.append(b)
            n_blob += b.size
        ctg_seg.append(len(segs))
        names.append(name)
        name_off.append(name_off[-1] + len(name))
    return (np.array(ctg_seg, np.uint64), np.array(segs, capi.SEG_SRC_DTYPE), np.concatenate(blob + [np.zeros(0, np.uint8)]), case["k"], case["line_length"],
            b"".join(names), np.array(name_off, np.uint64))


def layout(case):
    """the arrays the text kernel reads, laid out here: the segments back to back, oriented, in `sym`"""
    k, ll = case["k"], case["line_length"]
    ctg_text, ctg_seg, ctg_sym, name_off, seg_start, seg_off, skip, syms, names = [0], [0], [], [0], [], [], [], [], []
    n_sym_total = 0
    for name, segs in case["contigs"]:
        pos = 0
        for i, s in enumerate(segs):
            o = oriented(s)
            assert i == 0 or o.size >= k
            seg_start.append(pos)
            seg_off.append(n_sym_total)
            skip.append(0 if i == 0 else k)
            pos += o.size - skip[-1]
            n_sym_total += o.size
            syms.append(o)
        ctg_sym.append(pos)
        ctg_seg.append(len(seg_start))
        names.append(name)
        name_off.append(name_off[-1] + len(name))
        ctg_text.append(ctg_text[-1] + contig_text_size(len(name), pos, ll))
    u64 = lambda v: np.array(v, np.uint64)  # noqa: E731
    return {"ctg_text": u64(ctg_text), "ctg_seg": u64(ctg_seg), "ctg_sym": u64(ctg_sym), "name_off": u64(name_off), "names": b"".join(names),
            "seg_start": u64(seg_start), "seg_off": u64(seg_off), "skip": np.array(skip, np.uint32),
            "sym": np.concatenate(syms + [np.zeros(0, np.uint8)]), "total": ctg_text[-1]}


def text_offset(lay, case, c, p):
    """text offset of the symbol at position p of contig c"""
    L = case["line_length"] or int(lay["ctg_sym"][c])
    return int(lay["ctg_text"][c]) + int(lay["name_off"][c + 1] - lay["name_off"][c]) + 2 + p + p // L


def boundaries(lay, case):
    """text offsets of the first kept symbol of every segment that keeps one (but a contig's first)"""
    out = []
    for c in range(len(case["contigs"])):
        a, b = int(lay["ctg_seg"][c]), int(lay["ctg_seg"][c + 1])
        for s in range(a + 1, b):
            end = int(lay["seg_start"][s + 1]) if s + 1 < b else int(lay["ctg_sym"][c])
            if end > int(lay["seg_start"][s]):
                out.append(text_offset(lay, case, c, int(lay["seg_start"][s])))
    return out


def _name(i, n):
    return (b"c%d " % i + b"name with blanks and more " * 13)[:n]


def _mutated(rng, ref, lo, n, **kw):
    """a stretch of ref with substitutions (and what **kw adds) that differs from the whole reference: its delta is never empty"""
    t = synth.mutate(rng, ref[lo:lo + n], 0.02, **kw)
    if t.size == ref.size and np.array_equal(t, ref):
        t[0] ^= 1
    return t


def _split_raw(rng, sym, k, n_seg):
    """sym cut into n_seg RAW segments; each but the first starts with k overlap symbols of its own (codes 4: they must not show)"""
    cuts = np.sort(rng.integers(0, sym.size + 1, size=n_seg - 1)) if n_seg > 1 else []
    parts = np.split(sym, cuts)
    out = []
    for i, p in enumerate(parts):
        stored = p if i == 0 else np.concatenate([np.full(k, 4, np.uint8), p])
        rc = int(rng.integers(0, 2))
        out.append(seg(RAW, rev_comp(stored) if rc else stored, rc))  # (stored so that its orientation gives the part)
    return out


def grid_cases():
    """every line length x the symbol counts around it, names of every length"""
    rng = np.random.default_rng(701)
    out = []
    for ll in LINE_LENGTHS:
        L = ll if 0 < ll < 1000 else 23
        contigs = []
        for i, n in enumerate((0, 1, L - 1, L, L + 1, 2 * L, 16 * L + 5)):
            sym = rng.integers(0, 16, size=n, dtype=np.uint8)
            contigs.append((_name(i, NAME_LENGTHS[(i + len(out)) % 6]), _split_raw(rng, sym, 17, 1 + i % 3) if n else ([] if i % 2 else [seg(RAW, sym)])))
        contigs.append((_name(7, 300), []))  # no segment at all: the header only
        out.append({"name": f"grid_ll{ll}", "k": 17, "line_length": ll, "refs": [], "contigs": contigs})
    return out


def zero_keep_case(k=17, line_length=16):
    """segments of exactly k symbols keep nothing: one, two in a row, one as a contig's last; first segments shorter than k"""
    rng = np.random.default_rng(702)
    ref = synth.random_seq(rng, 2000)
    r = lambda n: rng.integers(0, 16, size=n, dtype=np.uint8)  # noqa: E731
    z_raw = lambda rc: seg(RAW, np.full(k, 5, np.uint8), rc)  # noqa: E731
    z_delta = lambda rc: seg(DELTA, _mutated(rng, ref, 300, k), rc, 0)  # noqa: E731
    contigs = [
        (b"one", [seg(RAW, r(50)), z_raw(0), seg(RAW, r(40 + k), 1)]),
        (b"two in a row", [seg(RAW, r(50), 1), z_raw(1), z_delta(0), seg(DELTA, _mutated(rng, ref, 0, 900), 0, 0)]),
        (b"the last one", [seg(DELTA, _mutated(rng, ref, 100, 500), 1, 0), seg(RAW, r(30 + k)), z_delta(1)]),
        (b"nothing but", [seg(RAW, r(33)), z_raw(0), z_raw(1), z_delta(0)]),
        (b"short first", [seg(RAW, r(k - 5)), seg(RAW, r(40 + k))]),
        (b"short first alone", [seg(RAW, r(3), 1)]),
        (b"first of exactly k", [seg(RAW, r(k)), z_raw(0), seg(RAW, r(k + 1))]),
        (b"empty first", [seg(RAW, r(0)), seg(RAW, r(k + 20))]),
    ]
    return {"name": f"zero_keep_k{k}", "k": k, "line_length": line_length, "refs": [ref], "contigs": contigs}


def boundary_case(line_length):
    """segments that keep 33 symbols each behind a body that starts on a chunk boundary: their boundaries fall on every chunk offset
    (17 boundaries do on one line; with line ends in between it takes 30)"""
    rng = np.random.default_rng(703)
    k = 31
    n_seg = 31 if line_length else 18
    refs = [synth.random_seq(rng, 33 + k) for _ in range(n_seg // 3 + 1)] + [synth.random_seq(rng, 3000)]
    segs = []
    for i in range(n_seg):
        n = 33 + (k if i else 0)
        kind = (RAW, REF, DELTA)[i % 3]
        rc = (i // 3) % 2
        if kind == RAW or i == 0:
            segs.append(seg(RAW, rng.integers(0, 16, size=n, dtype=np.uint8), rc))
        elif kind == REF:
            segs.append(seg(REF, refs[i // 3], rc, i // 3))
        else:
            segs.append(seg(DELTA, _mutated(rng, refs[-1], 40 * i, n), rc, len(refs) - 1))
    return {"name": f"boundary_ll{line_length}", "k": k, "line_length": line_length, "refs": refs, "contigs": [(_name(0, 14), segs)]}


def kinds_case():
    """all three kinds in both orientations; a reference with an escaped block (N-run, IUPAC codes); codes >= 16 in RAW segments"""
    rng = np.random.default_rng(704)
    k = 25
    clean = synth.random_seq(rng, 3000)
    esc = synth.random_seq(rng, 3000)
    esc[1100:1140] = 4
    esc[[5, 1500, 2999]] = (7, 15, 11)
    odd = rng.integers(0, 4, size=300, dtype=np.uint8)
    odd[[0, 17, 100, 101, 299]] = (16, 20, 30, 255, 31)
    segs = [seg(REF, clean, 0, 0)]
    for rc in (1, 0):
        segs += [seg(REF, esc, rc, 1), seg(DELTA, _mutated(rng, clean, 10, 2500, n_runs=2), rc, 0), seg(RAW, odd, rc),
                 seg(DELTA, _mutated(rng, esc, 0, 3000, n_runs=2, iupac=3, indels=2), rc, 1), seg(REF, clean, rc, 0)]
    other = [seg(RAW, odd, 1), seg(DELTA, _mutated(rng, esc, 900, 600), 1, 1)]
    return {"name": "kinds", "k": k, "line_length": 60, "refs": [clean, esc], "contigs": [(b"all kinds", segs), (b"raw first, reversed", other)]}


def many_case():
    """about 1000 contigs of 0..200 symbols in one call"""
    rng = np.random.default_rng(705)
    k = 21
    ref = synth.random_seq(rng, 400)
    contigs = []
    for i in range(1000):
        n = int(rng.integers(0, 201))
        if i % 7 == 3 and n > k:
            segs = [seg(DELTA, _mutated(rng, ref, int(rng.integers(0, 100)), n, n_runs=i % 2), i % 2, 0), seg(RAW, np.full(k, 4, np.uint8))]
        else:
            segs = _split_raw(rng, rng.integers(0, 5, size=n, dtype=np.uint8), k, 1 + i % 3)
        contigs.append((_name(i, int(rng.integers(1, 40))), segs))
    return {"name": "many", "k": k, "line_length": 80, "refs": [ref], "contigs": contigs}


def big_case(k, line_length):
    """one contig of about 1.2 M symbols in 40 segments"""
    rng = np.random.default_rng(706 + k)
    n = 30_000
    refs = [synth.random_seq(rng, n + k) for _ in range(14)]
    segs = []
    for i in range(40):
        kind, rc = (DELTA, REF, RAW)[i % 3], (i // 3) % 2
        if kind == REF:
            segs.append(seg(REF, refs[i // 3], rc, i // 3))
        elif kind == DELTA:
            segs.append(seg(DELTA, _mutated(rng, refs[i // 3], 0, n + k, n_runs=2, indels=1), rc, i // 3))
        else:
            segs.append(seg(RAW, rng.integers(0, 5, size=n + k - i, dtype=np.uint8), rc))
    return {"name": f"big_k{k}", "k": k, "line_length": line_length, "refs": refs, "contigs": [(b"chr1 of the big case", segs)]}


def small_cases():
    return grid_cases() + [zero_keep_case(), zero_keep_case(32, 0), boundary_case(0), boundary_case(60), kinds_case(), many_case()]


def big_cases():
    return [big_case(17, 80), big_case(31, 0), big_case(32, 1)]


def check_preconditions(case, lay):
    """what an arrangement is there for, asserted on the plan itself"""
    name = case["name"]
    counts = [int(x) for x in lay["ctg_sym"]]
    if name.startswith("grid"):
        ll = case["line_length"]
        L = ll if 0 < ll < 1000 else 23
        assert counts[:7] == [0, 1, L - 1, L, L + 1, 2 * L, 16 * L + 5]
        assert ll != 5000 or max(counts) < ll
        assert {len(n) for n, _ in case["contigs"]} == set(NAME_LENGTHS)
    elif name.startswith("zero_keep"):
        k = case["k"]
        keeps = [[x.size for x in kept(s, k)] for _n, s in case["contigs"]]
        assert keeps[0][1] == 0 and keeps[0][2] > 0                           # one, between two that keep
        assert keeps[1][1] == 0 and keeps[1][2] == 0 and keeps[1][3] > 0      # two in a row
        assert keeps[2][-1] == 0 and keeps[2][-2] > 0                         # a contig's last
        assert keeps[3][1:] == [0, 0, 0]
        assert 0 < keeps[4][0] < k and 0 < keeps[5][0] < k and keeps[6][0] == k and keeps[7][0] == 0
    elif name.startswith("boundary"):
        assert text_offset(lay, case, 0, 0) % 16 == 0 or case["line_length"]
        assert {b % 16 for b in boundaries(lay, case)} == set(range(16))
    elif name == "kinds":
        seen = {(s["kind"], s["rc"]) for _n, segs in case["contigs"] for s in segs}
        assert seen == {(kd, rc) for kd in (RAW, REF, DELTA) for rc in (0, 1)}
        assert any((r > 3).any() for r in case["refs"]) and any((s["stored"] >= 16).any() for _n, segs in case["contigs"] for s in segs if s["kind"] == RAW)
    elif name == "many":
        assert len(counts) == 1000 and min(counts) == 0 and max(counts) <= 200
        starts = {text_offset(lay, case, c, 0) % 16 for c in range(1000)}
        assert starts == set(range(16))                                       # every alignment of a body start
    elif name.startswith("big"):
        assert len(counts) == 1 and 1_150_000 < counts[0] < 1_250_000 and len(case["contigs"][0][1]) == 40
