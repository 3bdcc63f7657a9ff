"""Inputs and checks for the BGZF coder tests (tests/test_bgzf_host.py, tests/test_gpu_bgzf.py): the cases at which the coder can go
wrong, the CPU build of agc_amd/csrc/bgzf.h (tests/bgzf_host), and a walk over a stream's members that checks each against zlib."""
import ctypes as C
import gzip
import zlib

import numpy as np

BLOCK = 65280
MEMBER_MAX = 65311
HEADER = bytes.fromhex("1f8b08040000000000ff0600424302 00".replace(" ", ""))  # the 16 fixed bytes in front of BSIZE
EOF_MEMBER = bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")


def bound(n):
    return n + 31 * ((n + BLOCK - 1) // BLOCK) + 28


def fasta_text(rng, n, line_length, n_runs=True):
    """FASTA text of at least n bytes cut to n: headers, upper and lower case, IUPAC codes and N runs, lines of line_length (0: one
    line per record)"""
    out = bytearray()
    i = 0
    while len(out) < n:
        m = int(rng.integers(500, 40000))
        seq = rng.choice(np.frombuffer(b"ACGT", np.uint8), m)
        lo = int(rng.integers(0, m))
        seq[lo:lo + int(rng.integers(0, 3000))] |= 0x20  # a lower-case stretch
        at = rng.integers(0, m, m // 400)
        seq[at] = rng.choice(np.frombuffer(b"RYSWKMBDHVN", np.uint8), at.size)
        if n_runs:
            lo = int(rng.integers(0, m))
            seq[lo:lo + int(rng.integers(0, 5000))] = ord("N")
        body = seq.tobytes()
        out += b">ctg%d sample/%d len=%d\n" % (i, i * 7, m)
        if line_length:
            out += b"\n".join(body[p:p + line_length] for p in range(0, m, line_length)) + b"\n"
        else:
            out += body + b"\n"
        i += 1
    return bytes(out[:n])


def acgt_text(rng, n, line_length=80):
    """uniform random ACGT in lines of line_length, no header"""
    rows = (n + line_length) // (line_length + 1) + 1
    a = rng.choice(np.frombuffer(b"ACGT", np.uint8), (rows, line_length + 1))
    a[:, line_length] = ord("\n")
    return a.tobytes()[:n]


def fibonacci_block():
    """22 distinct bytes with the counts F(1) .. F(22) (46 367 bytes, one block), shuffled: a Huffman code without a limit is 21 deep"""
    f = [1, 1]
    while len(f) < 22:
        f.append(f[-1] + f[-2])
    assert sum(f) == 46367
    a = np.repeat(np.arange(40, 62, dtype=np.uint8), f)
    np.random.default_rng(22).shuffle(a)
    return a.tobytes()


def cases():
    """name -> bytes"""
    rng = np.random.default_rng(4)
    text = fasta_text(rng, BLOCK + 1, 80)
    out = {
        "empty": b"",
        "one_byte": b"G",
        "one_letter_block": b"N" * BLOCK,
        "fasta_65279": text[:BLOCK - 1],
        "fasta_65280": text[:BLOCK],
        "fasta_65281": text[:BLOCK + 1],
        "random_bytes": bytes(rng.integers(0, 256, 2 * BLOCK + 777, dtype=np.uint8)),
        "fibonacci": fibonacci_block(),
        "fasta_ll0": fasta_text(rng, 150000, 0),
        "fasta_ll60": fasta_text(rng, 150000, 60),
        "fasta_ll80": fasta_text(rng, 150000, 80),
        "acgt_3_blocks": acgt_text(rng, 3 * BLOCK),
    }
    return out


def host_encoder():
    """the CPU build of the coder (tests/bgzf_host) -> run(data) -> (stream, block offsets: n_blocks + 1)"""
    from tests.bgzf_host import build as bgzf_build
    u8p, u64p = C.POINTER(C.c_uint8), C.POINTER(C.c_uint64)
    L = C.CDLL(bgzf_build.build())
    L.bgzf_host_encode.argtypes = [C.c_char_p, C.c_uint64, u8p, C.c_uint64, u64p, u64p]
    L.bgzf_host_bound.restype = C.c_uint64
    L.bgzf_host_bound.argtypes = [C.c_uint64]
    L.bgzf_host_block_unaligned.restype = C.c_uint32
    L.bgzf_host_block_unaligned.argtypes = [C.c_char_p, C.c_uint32, u8p]

    def run(data):
        data = bytes(data)
        cap = bound(len(data))
        assert L.bgzf_host_bound(len(data)) == cap
        n = C.c_uint64()
        short = np.full(max(cap - 1, 1), 0xAA, np.uint8)
        assert L.bgzf_host_encode(data, len(data), short.ctypes.data_as(u8p), cap - 1, C.byref(n), None) == -1 and n.value == cap and (short == 0xAA).all()
        out = np.full(cap + 16, 0xAA, np.uint8)
        off = np.zeros((len(data) + BLOCK - 1) // BLOCK + 1, np.uint64)
        assert L.bgzf_host_encode(data, len(data), out.ctypes.data_as(u8p), cap, C.byref(n), off.ctypes.data_as(u64p)) == 0
        assert n.value <= cap and (out[n.value:] == 0xAA).all()
        return out[:n.value].tobytes(), off

    def block_unaligned(block):
        out = np.zeros(65312, np.uint8)
        k = L.bgzf_host_block_unaligned(bytes(block), len(block), out.ctypes.data_as(u8p))
        return out[:k].tobytes()

    run.block_unaligned = block_unaligned
    return run


def walk(stream, data, block_off=None):
    """every member of the stream against its slice of data -> [(BTYPE, payload bytes, input bytes)] of the data members"""
    assert gzip.decompress(stream) == data
    n_blocks = (len(data) + BLOCK - 1) // BLOCK
    at, seen, offs = 0, [], []
    for b in range(n_blocks + 1):
        offs.append(at)
        assert stream[at:at + 16] == HEADER, (b, stream[at:at + 16].hex())
        size = int.from_bytes(stream[at + 16:at + 18], "little") + 1
        assert size <= MEMBER_MAX and at + size <= len(stream), (b, size)
        member = stream[at:at + size]
        if b == n_blocks:
            assert member == EOF_MEMBER and at + size == len(stream)  # BSIZE chains exactly to the EOF member at the stream's end
            break
        want = data[b * BLOCK:(b + 1) * BLOCK]
        payload = member[18:-8]
        d = zlib.decompressobj(-15)
        assert d.decompress(payload) + d.flush() == want and d.eof and not d.unused_data, b
        assert int.from_bytes(member[-8:-4], "little") == zlib.crc32(want), b
        assert int.from_bytes(member[-4:], "little") == len(want), b
        assert payload[0] & 1 == 1, b  # BFINAL
        seen.append(((payload[0] >> 1) & 3, len(payload), len(want)))
        at += size
    if block_off is not None:
        assert [int(x) for x in block_off] == offs
    return seen
