"""Streams and expectations for the BGZF inflate tests (tests/test_inflate_host.py, tests/test_gpu_inflate.py): members made with
Python's zlib (raw deflate) or assembled bit by bit, wrapped into the BGZF header and trailer by hand; the CPU build of
agc_amd/csrc/inflate.h (tests/inflate_host).

A case is a list of members (member bytes, the text it holds, the Why the decoder must answer -- 0: it inflates); its stream is the
members back to back.  Why mirrors agc_amd/csrc/inflate.h; the Status follows from it (status_of)."""
import ctypes as C
import gzip
import zlib

import numpy as np

WHY = ["OK", "HEADER_TRUNCATED", "MAGIC", "METHOD", "FLAGS", "NO_BC", "SUBFIELD", "BSIZE_SMALL", "BSIZE_PAST", "ISIZE",
       "BLOCK_TYPE", "STORED_LEN", "HLIT", "HDIST", "REPEAT_FIRST", "RUN_PAST", "NO_EOB", "OVERSUBSCRIBED", "INCOMPLETE", "NO_CODE", "LITLEN_SYMBOL",
       "DIST_SYMBOL", "DISTANCE", "OUT_PAST", "OUT_SHORT", "EXHAUSTED", "LEFT_OVER", "CRC"]
W = {n: i for i, n in enumerate(WHY)}
N_WALK = 10  # Why below this: the walk's
OK, UNSUPPORTED, MALFORMED = 0, 1, 2
EINVAL, ECAP = -2, -4
EOF_MEMBER = bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")
SIZES = [0, 1, 64, 65, 4096, 65280, 65536]


def status_of(why):
    return OK if why == 0 else UNSUPPORTED if why in (W["METHOD"], W["FLAGS"], W["NO_BC"]) else MALFORMED


# ---- members ---------------------------------------------------------------------------------------------------------------------------
def member(payload, text, extra_front=b"", flg=4, name=None, comment=None, crc=None, isize=None, bsize=None, cm=8):
    """the payload (raw deflate) as a BGZF member: the 12 fixed bytes, the extra field (extra_front: subfields in front of BC), FNAME /
    FCOMMENT when given, the payload, CRC-32 and ISIZE of text (or what crc / isize / bsize say instead)"""
    tail = b""
    if name is not None:
        flg |= 8
        tail += name + b"\0"
    if comment is not None:
        flg |= 16
        tail += comment + b"\0"
    xlen = len(extra_front) + 6
    size = 12 + xlen + len(tail) + len(payload) + 8
    bc = b"BC\x02\x00" + ((size - 1) if bsize is None else bsize).to_bytes(2, "little")
    head = bytes([0x1f, 0x8b, cm, flg, 0, 0, 0, 0, 0, 0xff]) + xlen.to_bytes(2, "little") + extra_front + bc + tail
    return head + payload + (zlib.crc32(text) if crc is None else crc).to_bytes(4, "little") + (len(text) if isize is None else isize).to_bytes(4, "little")


def deflate(text, level=6, strategy=zlib.Z_DEFAULT_STRATEGY, flush_at=None):
    """raw deflate (wbits -15); flush_at: a Z_FULL_FLUSH behind that many bytes (several blocks, an empty stored one among them)"""
    c = zlib.compressobj(level, zlib.DEFLATED, -15, 9, strategy)
    out = b""
    if flush_at is not None:
        out = c.compress(text[:flush_at]) + c.flush(zlib.Z_FULL_FLUSH)
        text = text[flush_at:]
    return out + c.compress(text) + c.flush()


class Bits:
    """a deflate bitstream written by hand: fields from bit 0 of a byte on, Huffman codes with their first bit first"""

    def __init__(self):
        self.v, self.n = 0, 0

    def put(self, value, nbits):
        self.v |= value << self.n
        self.n += nbits
        return self

    def code(self, code, nbits):
        for i in range(nbits - 1, -1, -1):
            self.put((code >> i) & 1, 1)
        return self

    def align(self):
        self.n = (self.n + 7) & ~7
        return self

    def raw(self, data):
        self.align()
        for b in data:
            self.put(b, 8)
        return self

    def bytes(self):
        return self.v.to_bytes((self.n + 7) // 8, "little")


def canonical(lengths):
    """code lengths -> {symbol: (code, length)} (RFC 1951, 3.2.2)"""
    code, out = 0, {}
    for bits in range(1, 16):
        for s, l in enumerate(lengths):
            if l == bits:
                out[s] = (code, bits)
                code += 1
        code <<= 1
    return out


FIXED_LIT = canonical([8] * 144 + [9] * 112 + [7] * 24 + [8] * 8)
FIXED_DIST = canonical([5] * 32)
CL_ORDER = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]
CL_LEN = [5] * 16 + [2, 3, 3]  # a complete code-length code with every symbol in it
CL_CODE = canonical(CL_LEN)
CL_EXTRA = {16: 2, 17: 3, 18: 7}


def dynamic_head(b, cl_syms, hlit, hdist, last=1):
    """the header of a dynamic block: cl_syms = the code-length symbols as they are sent, (symbol, extra bits' value) for 16 / 17 / 18"""
    b.put(last, 1).put(2, 2).put(hlit - 257, 5).put(hdist - 1, 5).put(19 - 4, 4)
    for s in CL_ORDER:
        b.put(CL_LEN[s], 3)
    for s in cl_syms:
        s, x = s if isinstance(s, tuple) else (s, 0)
        b.code(*CL_CODE[s])
        b.put(x, CL_EXTRA.get(s, 0))
    return b


def dynamic(lit_len, dist_len, body, last=1):
    """a dynamic block with these code lengths, sent one by one; body: ("lit", symbol) / ("dist", symbol) / ("x", value, bits)"""
    b = dynamic_head(Bits(), list(lit_len) + list(dist_len), len(lit_len), len(dist_len), last)
    lit, dist = canonical(lit_len), canonical(dist_len)
    for item in body:
        if item[0] == "x":
            b.put(item[1], item[2])
        else:
            b.code(*(lit if item[0] == "lit" else dist)[item[1]])
    return b


def lit_lengths(used):
    """code lengths over 257 symbols or more, {symbol: length} for the used ones"""
    out = [0] * max(257, max(used) + 1)
    for s, l in used.items():
        out[s] = l
    return out


def fixed(body, last=1):
    b = Bits().put(last, 1).put(1, 2)
    for item in body:
        if item[0] == "x":
            b.put(item[1], item[2])
        else:
            b.code(*(FIXED_LIT if item[0] == "lit" else FIXED_DIST)[item[1]])
    return b


# ---- texts -------------------------------------------------------------------------------------------------------------------------------
def texts(n):
    """kind -> n bytes"""
    rng = np.random.default_rng(n + 7)
    rows = n // 81 + 2
    acgt = rng.choice(np.frombuffer(b"ACGT", np.uint8), (rows, 81))
    acgt[:, 80] = 10
    block = rng.choice(np.frombuffer(b"ACGT", np.uint8), 32768).tobytes()
    out = {"acgt80": acgt.tobytes()[:n], "n_runs": (b"N" * 80 + b"\n") * (n // 81 + 1), "random": bytes(rng.integers(0, 256, n, dtype=np.uint8)),
           "block32k": block * 3}
    for p in (3, 7, 63, 64, 65):
        unit = bytes(rng.choice(np.frombuffer(b"ACGTN", np.uint8), p))
        out["period%d" % p] = unit * (n // p + 1)
    return {k: v[:n] for k, v in out.items()}


MODES = {"stored": dict(level=0), "level1": dict(level=1), "level6": dict(level=6), "level9": dict(level=9), "fixed": dict(strategy=zlib.Z_FIXED),
         "huffman_only": dict(strategy=zlib.Z_HUFFMAN_ONLY), "rle": dict(strategy=zlib.Z_RLE)}


def good(text, **kw):
    return (member(deflate(text, **kw), text), text, 0)


def hand_made():
    """name -> (member, text, why) for what zlib never emits"""
    rng = np.random.default_rng(11)
    far = bytes(rng.integers(65, 70, 32768, dtype=np.uint8))
    d32768 = Bits().put(0, 1).put(0, 2).align().put(32768, 16).put(32768 ^ 0xFFFF, 16).raw(far).bytes() + \
        fixed([("lit", 257), ("dist", 29), ("x", 8191, 13), ("lit", 256)]).bytes()
    # lengths 1, 2, .. 14, 15, 15 over 'A' .. 'O' and end-of-block: the last two codes have 15 bits
    deep = lit_lengths({**{65 + i: i + 1 for i in range(15)}, 256: 15})
    deep_text = bytes(rng.choice(np.arange(65, 80, dtype=np.uint8), 300, p=np.array([2.0 ** -(i + 1) for i in range(14)] + [2.0 ** -14])))
    deep_text += bytes(range(65, 80))
    one_dist = lit_lengths({65: 1, 256: 2, 257: 2})  # 'A', end-of-block, length 3
    no_dist = lit_lengths({65: 1, 66: 2, 256: 2})
    return {
        "distance_32768": (member(d32768, far + far[:3]), far + far[:3], 0),
        "code_of_15_bits": (member(dynamic(deep, [1, 1], [("lit", c) for c in deep_text] + [("lit", 256)]).bytes(), deep_text), deep_text, 0),
        "one_distance_code": (member(dynamic(one_dist, [1], [("lit", 65), ("lit", 257), ("dist", 0), ("lit", 256)]).bytes(), b"AAAA"), b"AAAA", 0),
        "no_distance_code": (member(dynamic(no_dist, [0], [("lit", 65), ("lit", 66), ("lit", 256)]).bytes(), b"AB"), b"AB", 0),
        "length_258_distance_1": (member(fixed([("lit", 71), ("lit", 285), ("dist", 0), ("lit", 256)]).bytes(), b"G" * 259), b"G" * 259, 0),
        "length_284_all_extra_bits": (member(fixed([("lit", 71), ("lit", 284), ("x", 31, 5), ("dist", 0), ("lit", 256)]).bytes(), b"G" * 259), b"G" * 259, 0),
    }


def refusals():
    """name -> (member, text, why): a good member with one mutation each"""
    text = texts(4096)["acgt80"]
    pay = deflate(text)
    stored = deflate(text, level=0)
    ok2 = lit_lengths({65: 1, 256: 2, 257: 2})
    out = {
        # the walk's
        "plain_gzip": (gzip.compress(text), text, W["NO_BC"]),
        "other_subfield_only": (member(pay, text)[:12] + b"XY" + member(pay, text)[14:], text, W["NO_BC"]),
        "method_9": (member(pay, text, cm=9), text, W["METHOD"]),
        "reserved_flag": (member(pay, text, flg=4 | 0x20), text, W["FLAGS"]),
        "bsize_too_small": (member(pay, text, bsize=20), text, W["BSIZE_SMALL"]),
        "bsize_past_the_input": (member(pay, text, bsize=65535), text, W["BSIZE_PAST"]),
        "isize_65537": (member(pay, text, isize=65537), text, W["ISIZE"]),
        "subfield_past_the_extra_field": (member(pay, text, extra_front=b"XY\xff\x00"), text, W["SUBFIELD"]),
        "header_truncated": (member(pay, text)[:11], text, W["HEADER_TRUNCATED"]),
        "not_a_member": (b"\0" * 30, text, W["MAGIC"]),
        # the member's
        "block_type_3": (member(Bits().put(1, 1).put(3, 2).bytes(), b""), b"", W["BLOCK_TYPE"]),
        "stored_len_nlen": (member(stored[:3] + bytes([stored[3] ^ 1]) + stored[4:], text), text, W["STORED_LEN"]),
        "hlit_287": (member(Bits().put(1, 1).put(2, 2).put(30, 5).put(0, 5).put(0, 4).put(0, 64).bytes(), b""), b"", W["HLIT"]),
        "hdist_31": (member(Bits().put(1, 1).put(2, 2).put(0, 5).put(30, 5).put(0, 4).put(0, 64).bytes(), b""), b"", W["HDIST"]),
        "repeat_without_a_length": (member(dynamic_head(Bits(), [(16, 0)] + [0] * 300, 257, 1).bytes(), b""), b"", W["REPEAT_FIRST"]),
        "run_past_the_lengths": (member(dynamic_head(Bits(), [1] + [0] * 250 + [(18, 127)], 257, 1).bytes(), b""), b"", W["RUN_PAST"]),
        "no_end_of_block": (member(dynamic(lit_lengths({65: 1, 66: 1}), [0], []).bytes(), b""), b"", W["NO_EOB"]),
        "oversubscribed": (member(dynamic(lit_lengths({65: 1, 66: 1, 256: 1}), [0], []).bytes(), b""), b"", W["OVERSUBSCRIBED"]),
        "incomplete": (member(dynamic(lit_lengths({65: 2, 256: 2}), [0], []).bytes(), b""), b"", W["INCOMPLETE"]),
        "incomplete_one_code": (member(dynamic(lit_lengths({256: 1}), [0], [("lit", 256)]).bytes(), b""), b"", W["INCOMPLETE"]),  # zlib takes this one
        "incomplete_distance_code": (member(dynamic(ok2, [2, 2], []).bytes(), b""), b"", W["INCOMPLETE"]),
        "oversubscribed_code_length_code": (member(Bits().put(1, 1).put(2, 2).put(0, 5).put(0, 5).put(0, 4).put(0o1111, 12).put(0, 64).bytes(), b""), b"", W["OVERSUBSCRIBED"]),
        "no_code_in_one_distance_code": (member(dynamic(ok2, [1], [("lit", 65), ("lit", 257), ("x", 1, 1), ("lit", 256)]).bytes(), b"AAAA"), b"AAAA", W["NO_CODE"]),
        "match_without_distance_code": (member(dynamic(ok2, [0], [("lit", 65), ("lit", 257), ("x", 0, 1), ("lit", 256)]).bytes(), b"AAAA"), b"AAAA", W["NO_CODE"]),
        "symbol_286": (member(fixed([("lit", 65), ("lit", 286)]).bytes(), b"A"), b"A", W["LITLEN_SYMBOL"]),
        "distance_symbol_30": (member(fixed([("lit", 65), ("lit", 257), ("dist", 30), ("lit", 256)]).bytes(), b"AAAA"), b"AAAA", W["DIST_SYMBOL"]),
        "distance_beyond_the_output": (member(fixed([("lit", 65), ("lit", 257), ("dist", 1), ("lit", 256)]).bytes(), b"AAAA"), b"AAAA", W["DISTANCE"]),
        "output_past_isize": (member(pay, text, isize=len(text) - 1), text[:-1], W["OUT_PAST"]),
        "match_past_isize": (member(fixed([("lit", 71), ("lit", 285), ("dist", 0), ("lit", 256)]).bytes(), b"G" * 259, isize=200), b"G" * 200, W["OUT_PAST"]),
        "stored_past_isize": (member(stored, text, isize=100), text[:100], W["OUT_PAST"]),
        "output_short_of_isize": (member(pay, text, isize=len(text) + 1), text + b"?", W["OUT_SHORT"]),
        "payload_exhausted": (member(pay[:-3], text), text, W["EXHAUSTED"]),
        "payload_exhausted_in_the_header": (member(pay[:2], text), text, W["EXHAUSTED"]),
        "stored_payload_exhausted": (member(stored[:-1], text), text, W["EXHAUSTED"]),
        "payload_empty": (member(b"", b""), b"", W["EXHAUSTED"]),
        "payload_left_over": (member(pay + b"\0", text), text, W["LEFT_OVER"]),
        "crc_mismatch": (member(pay, text, crc=zlib.crc32(text) ^ 0x100), text, W["CRC"]),
    }
    return out


def cases():
    """name -> list of (member, text, why)"""
    out = {"empty_stream": [], "eof_member_alone": [(EOF_MEMBER, b"", 0)]}
    by_size = {n: texts(n) for n in SIZES}
    for kind in by_size[SIZES[0]]:
        for mode, kw in MODES.items():
            # (a member is 65536 bytes at most -- BSIZE has 16 bits --, so 65536 bytes of text come only where they compress)
            fits = [n for n in SIZES if len(deflate(by_size[n][kind], **kw)) + 26 <= 65536]
            assert fits[:6] == SIZES[:6]
            out["%s_%s" % (kind, mode)] = [good(by_size[n][kind], **kw) for n in fits] + [(EOF_MEMBER, b"", 0)]
    t = by_size[65280]
    out["full_flush_in_the_middle"] = [good(t["acgt80"], flush_at=30000), good(t["period7"], flush_at=0), good(t["random"], level=1, flush_at=65279), (EOF_MEMBER, b"", 0)]
    small = by_size[4096]["acgt80"]
    pay = deflate(small)
    out["second_subfield_in_front_of_bc"] = [(member(pay, small, extra_front=b"XY\x03\x00abc"), small, 0), (member(pay, small, extra_front=b"BC\x01\x00zAB\x00\x00"), small, 0)]
    out["name_and_comment"] = [(member(pay, small, name=b"sample.fa"), small, 0), (member(pay, small, comment=b"a comment"), small, 0),
                               (member(pay, small, name=b"", comment=b"c"), small, 0), (member_fhcrc(pay, small), small, 0)]
    for name, m in hand_made().items():
        out[name] = [good(small), m, good(small, level=1)]
    # about 70 members of mixed kinds; with and without the EOF member
    rng = np.random.default_rng(70)
    kinds, modes = list(by_size[4096]), list(MODES)
    mixed = []
    for i in range(70):
        n = int(rng.choice([0, 1, 64, 65, 4096, 777, 30000]))
        mixed.append(good(texts(n)[kinds[i % len(kinds)]], **MODES[modes[(i * 3) % len(modes)]]))
    out["mixed_70_members"] = mixed + [(EOF_MEMBER, b"", 0)]
    out["mixed_70_members_no_eof"] = mixed
    for name, m in refusals().items():
        out["refused_" + name] = [good(small), m] + ([] if name == "header_truncated" else [good(small, level=9), (EOF_MEMBER, b"", 0)])
    return out


def member_fhcrc(payload, text):
    """a member with FTEXT and FHCRC set: two more header bytes in front of the payload"""
    m = bytearray(member(b"\0\0" + payload, text))
    m[3] |= 2 | 1
    return bytes(m)


def bgzf_host_streams():
    """name -> [(member, text, 0)] of the streams tests/bgzf_host's CPU coder writes (dynamic blocks with two unused distance codes, stored ones)"""
    from tests import bgzf_cases as BC
    enc = BC.host_encoder()
    out = {}
    for name, data in BC.cases().items():
        stream, off = enc(data)
        ends = [int(x) for x in off[1:]] + [len(stream)]
        out["bgzf_host_" + name] = [(stream[int(a):b], data[i * BC.BLOCK:(i + 1) * BC.BLOCK], 0) for i, (a, b) in enumerate(zip(off, ends))]
    return out


def expect(case):
    """-> (stream, return code, the members' texts -- None when the walk complains --, statuses, whys, text_off): what
    agc_hip_bgzf_inflate must answer (a refused member's range has unspecified contents: compare with same_text)"""
    stream = b"".join(m for m, _t, _w in case)
    whys = []
    for _m, _t, w in case:
        whys.append(w)
        if 0 < w < N_WALK:
            break
    walk_bad = bool(whys) and 0 < whys[-1] < N_WALK
    members = case[:len(whys) - 1] if walk_bad else case
    off = np.cumsum([0] + [len(t) for _m, t, _w in members]).astype(np.uint64)
    rc = EINVAL if any(whys) else 0
    return stream, rc, (None if walk_bad else [t for _m, t, _w in members]), [status_of(w) for w in whys], whys, off


def same_text(got, case_texts, whys, off):
    """the good members' ranges of `got` hold their texts (a refused member's range is unspecified)"""
    assert len(got) == int(off[-1])
    for t, w, a in zip(case_texts, whys, off):
        assert w != 0 or bytes(got[int(a):int(a) + len(t)]) == t


# ---- the CPU build -------------------------------------------------------------------------------------------------------------------------
def host():
    """the CPU build of the decoder (tests/inflate_host) -> run(stream, cap=None) -> (rc, text bytes, text_off, statuses, whys); run.walk"""
    from tests.inflate_host import build as ib
    u8p, u32p, u64p = C.POINTER(C.c_uint8), C.POINTER(C.c_uint32), C.POINTER(C.c_uint64)
    L = C.CDLL(ib.build())
    L.inflate_host_stream.argtypes = [C.c_char_p, C.c_uint64, u8p, C.c_uint64, u64p, u64p, u32p, u32p]
    L.inflate_host_walk.restype = C.c_uint32
    L.inflate_host_walk.argtypes = [C.c_char_p, C.c_uint64, u64p, u32p, C.c_uint64, u64p, u64p, u32p, u64p]

    def walk(stream):
        """-> (status, why, at, members, text bytes, jobs[members][4]: src_off, out_off, src_len, out_len, crcs)"""
        cap = len(stream) // 26 + 1
        jobs, crcs = np.zeros((cap, 4), np.uint64), np.zeros(cap, np.uint32)
        nm, tb, at, why = C.c_uint64(), C.c_uint64(), C.c_uint64(), C.c_uint32()
        st = L.inflate_host_walk(stream, len(stream), jobs.ctypes.data_as(u64p), crcs.ctypes.data_as(u32p), cap, C.byref(nm), C.byref(tb), C.byref(why), C.byref(at))
        return st, why.value, at.value, nm.value, tb.value, jobs[:nm.value], crcs[:nm.value]

    def run(stream, cap=None):
        _st, _why, _at, nm, tb, _j, _c = walk(stream)
        cap = tb if cap is None else cap
        out = np.full(cap + 32, 0xAA, np.uint8)
        off, st, why = np.zeros(nm + 2, np.uint64), np.zeros(nm + 1, np.uint32), np.zeros(nm + 1, np.uint32)
        ln = C.c_uint64()
        rc = L.inflate_host_stream(stream, len(stream), out.ctypes.data_as(u8p), cap, C.byref(ln), off.ctypes.data_as(u64p), st.ctypes.data_as(u32p), why.ctypes.data_as(u32p))
        assert (out[cap:] == 0xAA).all()
        k = nm + 1 if _st else nm
        return rc, out[:ln.value].tobytes() if rc != ECAP else b"", off[:nm + 1], st[:k].tolist(), why[:k].tolist()

    run.walk = walk
    return run
