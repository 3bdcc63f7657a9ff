"""The shapes tests/test_parts_unpack_host.py (the CPU build of agc_amd/csrc/parts_unpack.h) and tests/test_gpu_sample_parts.py (the
kernels) are run on, and the plain numpy restatements they are compared with: a pack cut at its 0xFF terminators (nth_in_pack), a
tuple stream into its symbols (tuples2bytes, with the two checks it lacks)."""
import numpy as np

OK, ZD_UNSUPPORTED, ZD_MALFORMED, BAD_TUPLES = 0, 1, 2, 3
BASE = {2: 16, 3: 6, 4: 4}


# ---- packs ---------------------------------------------------------------------------------------------------------------------------
def pack_ends(pack):
    """offsets of the terminators = where the sequences end; bytes behind the last one belong to no sequence"""
    return np.flatnonzero(np.frombuffer(bytes(pack), np.uint8) == 0xFF).astype(np.uint32)


def pack_sequences(pack):
    pack = bytes(pack)
    out, start = [], 0
    for e in pack_ends(pack).tolist():
        out.append(pack[start:e])
        start = e + 1
    return out


def pack_of(seqs, tail=b""):
    return b"".join(bytes(s) + b"\xff" for s in seqs) + bytes(tail)


def _filler(n, seed=0):
    return np.random.default_rng(1000 + n + seed).integers(0, 255, n, dtype=np.uint8).tobytes()  # (never 0xFF)


def pack_shapes():
    """[(name, pack bytes)]"""
    out = [("empty", b""), ("one terminator", b"\xff"), ("no terminator", _filler(200)), ("trailing bytes", pack_of([b"AB", b"CDE"], b"xyz")),
           ("two in a row", b"A\xff\xffB\xff"), ("three in a row", b"\xff\xff\xffA\xff"), ("only terminators", b"\xff" * 70)]
    for at in (15, 16, 17, 63, 64, 65, 1023, 1024, 1025):  # the lanes' and the strips' edges
        out.append((f"terminator at {at}", _filler(at) + b"\xff" + _filler(40, at)))
    for n in (64, 65, 128, 1024, 1040):
        out.append((f"last byte of {n}", _filler(n - 1) + b"\xff"))
    rng = np.random.default_rng(5)
    out.append(("three strips", pack_of([_filler(int(n), i) for i, n in enumerate(rng.integers(0, 120, 50))], b"tail")))
    return out


def capped_packs(seq_cap):
    """exactly seq_cap and seq_cap + 1 sequences"""
    return [(f"{n} sequences at cap {seq_cap}", pack_of([_filler(7 * i % 23, i) for i in range(n)])) for n in (seq_cap, seq_cap + 1)]


# ---- tuples --------------------------------------------------------------------------------------------------------------------------
def tuples_of(sym, nb):
    """bytes2tuples_impl (src/common/segment.h:114-138) for nb in 2, 3, 4; nb = 1: the pass-through form (symbols + marker 0x10)"""
    sym = np.asarray(sym, np.uint8)
    if nb == 1:
        return sym.tobytes() + b"\x10"
    base, out = BASE[nb], bytearray()
    whole = sym.size // nb * nb
    for i in range(0, whole, nb):
        c = 0
        for j in range(nb):
            c = c * base + int(sym[i + j])
        out.append(c)
    c = 0
    for v in sym[whole:].tolist():
        c = c * base + v
    out.append(c)
    out.append((nb << 4) + sym.size % nb)
    return bytes(out)


def symbols_of(t):
    """tuples2bytes, digit by digit -> the symbols (uint8), or None where the stream is refused"""
    t = bytes(t)
    if len(t) < 2:
        return None
    nb, last = t[-1] >> 4, t[-1] & 15
    if nb not in BASE:
        return np.frombuffer(t[:-1], np.uint8).copy()
    if last > nb:
        return None
    n = (len(t) - 2) * nb + last
    out = np.zeros(n, np.uint8)
    for q in range(-(-n // nb)):
        digits, c = min(nb, n - q * nb), t[q]
        for k in range(digits - 1, -1, -1):
            out[q * nb + k] = c % BASE[nb]
            c //= BASE[nb]
    return out


def symbol_counts(nb):
    return sorted({0, 1, nb - 1, nb, nb + 1, 15, 16, 17, 16 * nb - 1, 16 * nb + 1, 1000})


def tuple_shapes():
    """[(name, stream, its symbols)]: the writer's streams for every nb and count, and every legal low nibble on a fixed stream"""
    out = []
    for nb in (2, 3, 4, 1):
        for n in symbol_counts(nb)[1 if nb == 1 else 0:]:  # (no symbols at all: the writer takes nb 4, and a marker alone is refused)
            sym = np.random.default_rng(nb * 10000 + n).integers(0, 4 if nb == 4 else 6 if nb == 3 else 16 if nb == 2 else 200, n, dtype=np.uint8)
            t = tuples_of(sym, nb)
            assert np.array_equal(symbols_of(t), sym)
            out.append((f"nb {nb}, {n} symbols", t, sym))
    body = np.random.default_rng(77).integers(0, 256, 9, dtype=np.uint8).tobytes()
    for nb in (2, 3, 4):
        for last in range(nb + 1):  # (last == nb: the form the writer never makes, and tuples2bytes reads correctly)
            t = body + bytes([nb << 4 | last])
            out.append((f"nb {nb}, low nibble {last}", t, symbols_of(t)))
    for marker in (0x00, 0x10, 0x5F, 0xFF):
        t = body + bytes([marker])
        out.append((f"pass-through marker {marker:#x}", t, np.frombuffer(body, np.uint8)))
    return out


def refused_tuples():
    """[(name, stream)]: what the host routine would read or write outside its buffers for"""
    body = bytes(range(40, 52))
    out = [("size 0", b""), ("size 1", b"\x42")]
    for nb in (2, 3, 4):
        out += [(f"nb {nb}, low nibble {nb + 1}", body + bytes([nb << 4 | (nb + 1)])), (f"nb {nb}, low nibble 15", body + bytes([nb << 4 | 15]))]
    return out
