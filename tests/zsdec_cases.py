"""Frames for the zstd decoder tests (tests/test_zstd_decode_host.py, tests/test_gpu_zstd_decode.py): libzstd's ZSTD_decompress as
the oracle, a walk over a frame's headers that names what the frame contains, and the inputs that make libzstd emit each shape."""
import ctypes as C

import numpy as np

from tests import zstd_cases

LEVELS = (1, 3, 13, 17, 19)
MAGIC = 0xFD2FB528
OK, UNSUPPORTED, MALFORMED = 0, 1, 2


def _z():
    Z = zstd_cases.libzstd()
    if not getattr(Z, "_dec_bound", False):
        Z.ZSTD_decompress.restype = C.c_size_t
        Z.ZSTD_decompress.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t]
        Z.ZSTD_isError.restype = C.c_uint
        Z.ZSTD_isError.argtypes = [C.c_size_t]
        Z._dec_bound = True
    return Z


def ref_decode(frame, cap):
    """ZSTD_decompress into cap bytes -> the bytes, or None when libzstd refuses the input"""
    Z = _z()
    out = C.create_string_buffer(max(cap, 1))
    k = Z.ZSTD_decompress(out, cap, bytes(frame), len(frame))
    return None if Z.ZSTD_isError(k) else out.raw[:k]


def walk(frame):
    """the names of what a frame contains, from its frame header, block headers, literals headers (with the first byte of a
    Huffman tree description: direct or FSE-compressed weights) and sequence headers (count and mode byte) alone"""
    f = bytes(frame)
    feats = set()
    assert int.from_bytes(f[:4], "little") == MAGIC
    fhd = f[4]
    fcs_flag, single, did = fhd >> 6, (fhd >> 5) & 1, fhd & 3
    feats.add("hdr_single" if single else "hdr_window")
    pos = 5 + (0 if single else 1) + (4 if did == 3 else did)
    nfcs = (1 if single else 0) if fcs_flag == 0 else (2, 4, 8)[fcs_flag - 1]
    feats.add("fcs%d" % nfcs)
    content = int.from_bytes(f[pos:pos + nfcs], "little") + (256 if nfcs == 2 else 0)
    pos += nfcs
    if content == 0:
        feats.add("frame_empty")
    n_blocks = 0
    while True:
        bh = int.from_bytes(f[pos:pos + 3], "little")
        pos += 3
        last, btype, size = bh & 1, (bh >> 1) & 3, bh >> 3
        n_blocks += 1
        feats.add(("blk_raw", "blk_rle", "blk_comp")[btype])
        if btype == 2:
            _walk_block(f[pos:pos + size], feats)
        pos += 1 if btype == 1 else size
        if last:
            break
    assert pos == len(f)
    if n_blocks > 1:
        feats.add("blocks_many")
    return feats


def _walk_block(b, feats):
    b0 = b[0]
    ltype, sf = b0 & 3, (b0 >> 2) & 3
    feats.add(("lit_raw", "lit_rle", "lit_comp", "lit_treeless")[ltype])
    if ltype < 2:
        lh = (1, 2, 1, 3)[sf]
        size = int.from_bytes(b[:lh], "little") >> (3 if lh == 1 else 4)
        feats.add("lit_size_format%d" % lh)
        used = lh + (size if ltype == 0 else 1)
    else:
        lh = (3, 3, 4, 5)[sf]
        v = int.from_bytes(b[:lh], "little")
        bits = (10, 10, 14, 18)[sf]
        csize = (v >> (4 + bits)) & ((1 << bits) - 1)
        feats.add("streams1" if sf == 0 else "streams4")
        feats.add("lit_csize_format%d" % lh)
        tree = 0
        if ltype == 2:
            feats.add("weights_direct" if b[lh] >= 128 else "weights_fse")
            tree = 1 + ((b[lh] - 127 + 1) // 2 if b[lh] >= 128 else b[lh])
        if sf and len({int.from_bytes(b[lh + tree + 2 * i:lh + tree + 2 * i + 2], "little") for i in range(3)}) > 1:
            feats.add("streams4_uneven")  # (the jump table: the sizes of the first three streams)
        used = lh + csize
    s = b[used:]
    n = s[0]
    k = 1
    if n == 0:
        feats.add("seq_none")
        return
    if n < 128:
        feats.add("seq_count1")
    elif n < 255:
        feats.add("seq_count2")
        k = 2
    else:
        feats.add("seq_count3")
        k = 3
    modes = s[k]
    for name, m in (("ll", modes >> 6), ("of", (modes >> 4) & 3), ("ml", (modes >> 2) & 3)):
        feats.add(name + "_" + ("predefined", "rle", "fse", "repeat")[m])


# what the corpus of the host test must contain before anything is compared
REQUIRED = (["blk_raw", "blk_rle", "blk_comp", "lit_raw", "lit_rle", "lit_comp", "lit_treeless", "streams1", "streams4", "weights_direct", "weights_fse",
             "seq_none", "frame_empty", "hdr_single", "hdr_window", "blocks_many"]
            + [t + "_" + m for t in ("ll", "of", "ml") for m in ("predefined", "rle", "fse", "repeat")])


def _text(rng, n):
    words = [bytes(rng.integers(97, 123, int(rng.integers(2, 9)), dtype=np.uint8)) for _ in range(150)]
    out = bytearray()
    while len(out) < n:
        out += words[int(rng.integers(len(words)))] + b" "
    return bytes(out[:n])


def _pack(oracle, rng, n):
    out = bytearray()
    while len(out) < n:
        out += zstd_cases.delta_pack(oracle, rng, 40, 60000, 3e-3)
    return bytes(out[:n])


def multi_block_inputs(oracle):
    """inputs of more than one block: the sizes around the block size and beyond, a match that reaches back across a block
    boundary, a run of one byte that spans blocks -> [(name, bytes)]"""
    rng = np.random.default_rng(77)
    pack, text = _pack(oracle, rng, 1000000), _text(rng, 1000000)
    out = []
    for n in (131072, 131073, 300000, 1000000):
        out.append(("pack_%d" % n, pack[:n]))
        out.append(("text_%d" % n, text[:n]))
    noise = bytes(rng.integers(0, 256, 131072, dtype=np.uint8))
    out.append(("match_across_blocks", noise + noise[-6000:] + text[:3000] + noise[100000:104000]))
    out.append(("run_across_blocks", b"\x07" * 400000))
    out.append(("run_then_text", b"\x00" * 140000 + text[:5000] + b"\x00" * 140000))
    return out


def feature_inputs():
    """inputs for the features the mixed corpus does not make libzstd emit: RLE literals, direct Huffman weights, a block without
    sequences, RLE and repeat mode of the sequence tables, a second block that is an RLE block -> [(name, bytes)]"""
    rng = np.random.default_rng(9)
    noise = bytes(rng.integers(0, 256, 131072, dtype=np.uint8))
    text = _text(rng, 140000)
    words3 = [bytes(rng.integers(0, 256, 3, dtype=np.uint8)) for _ in range(48)]
    return [
        # a second block of matches into the first with one and the same byte between them: RLE literals, RLE offsets / match lengths
        ("sep_block2", noise + b"".join(noise[70000 + 97 * i:70000 + 97 * i + 40] + b"\x00" for i in range(300))),
        ("sep_block2_var", noise + b"".join(noise[1000 + 397 * i:1000 + 397 * i + 30 + (i % 5)] + bytes([i % 7]) for i in range(300))),
        ("acgt", bytes(rng.integers(0, 4, 6000, dtype=np.uint8))),            # four literal symbols: direct weights
        ("alpha16", bytes(rng.integers(0, 16, 300, dtype=np.uint8) * 16)),    # Huffman literals, no match: 0 sequences
        ("text_tail300", text[:131072 + 300]),                                # a small block behind a full one: repeat mode
        ("text_tail2000", text[:131072 + 2000]),
        ("two_runs", b"\x07" * 262144),                                       # the second block is an RLE block
        # 3-byte words with a byte between them: as many sequences in a block as libzstd can be made to write
        ("many_sequences", b"".join(words3[int(i)] + bytes([int(j)]) for i, j in zip(rng.integers(0, 48, 32768), rng.integers(0, 256, 32768)))),
    ]


def shape_inputs():
    """the smallest inputs that make libzstd emit each shape the device test needs -> {name: bytes}"""
    rng = np.random.default_rng(5)
    noise = bytes(rng.integers(0, 256, 4000, dtype=np.uint8))
    text = _text(rng, 300000)
    out = {
        "empty": b"",
        "one_byte": b"x",
        "rle_block": b"Q" * 262144,  # (libzstd never writes a frame's FIRST block as an RLE block: the second one is)
        "raw_block": noise,
        "offset1_long": noise[:50] + b"z" * 300 + noise[50:80],
        "treeless": text[:300000],
        "cross_block_match": noise * 32 + noise[3000:] + noise[:1000] + noise[2000:3500],
        "four_streams": text[:20000],
    }
    for off in (63, 64, 65):  # a period of `off` bytes repeated: one long match with that offset
        out["offset%d" % off] = noise[:off] * 6 + noise[100:120]
    for ll in (0, 1, 63, 64, 65):  # literal runs of ll bytes between matches of a block seen before
        blk = noise[200:400]
        out["litrun%d" % ll] = blk + b"".join(noise[1000 + 70 * i:1000 + 70 * i + ll] + blk[10 * i:10 * i + 60] for i in range(8)) + blk[:ll]
    return out


def host_decoder():
    """the CPU build of the decoder (tests/zsdec_host) -> run(frame) -> (status, bytes or None)"""
    from tests.zsdec_host import build as zsdec_build
    u8p = C.POINTER(C.c_uint8)
    L = C.CDLL(zsdec_build.build())
    L.zsdec_decode.restype = C.c_uint32
    L.zsdec_decode.argtypes = [C.c_char_p, C.c_uint64, u8p, C.c_uint64, C.POINTER(C.c_uint64)]
    assert L.zsdec_check_tables() == 0, "LLbase / MLbase are not the inverse of LLcode / MLcode"

    def run(frame):
        frame = bytes(frame)
        n = C.c_uint64()
        st = L.zsdec_decode(frame, len(frame), None, 0, C.byref(n))
        if st:
            return st, None
        out = np.full(n.value + 8, 0xAA, np.uint8)
        st = L.zsdec_decode(frame, len(frame), out.ctypes.data_as(u8p), n.value, C.byref(n))
        assert (out[n.value:] == 0xAA).all()
        return st, (None if st else out[:n.value].tobytes())
    return run


def archive_frames(path):
    """the zstd parts of an .agc archive's segment streams (x<id>r: a group's reference, x<id>d: its packs), each without the
    marker byte that follows the frame (agc_amd/csrc/host/archive_read.h: decode_ref_part / decode_pack_part) -> [(stream, frame)]"""
    from tests import agc_container
    streams, order = agc_container.parse(open(path, "rb").read())
    out = []
    for name in order:
        if name.startswith("x") and name[-1] in "rd":
            out += [(name, payload[:-1]) for meta, payload, _off in streams[name] if meta != 0 and len(payload) > 1]
    return out


def mutate(rng, frame):
    """one seeded mutation of a frame: a byte changed, a truncation, bytes appended"""
    m = bytearray(frame)
    t = int(rng.integers(8))
    if t < 4 and m:
        m[int(rng.integers(len(m)))] ^= 1 << int(rng.integers(8))
    elif t < 6 and m:
        del m[int(rng.integers(len(m))):]
    elif t == 6:
        m += bytes(rng.integers(0, 256, int(rng.integers(1, 9)), dtype=np.uint8))
    elif m:
        for _ in range(int(rng.integers(1, 5))):
            m[int(rng.integers(len(m)))] = int(rng.integers(256))
    return bytes(m)
