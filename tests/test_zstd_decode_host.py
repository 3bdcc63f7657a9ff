"""CPU: the zstd decoder of agc_amd/csrc/zstd/zs_decode.h (the header zstd_decode_kernel is built from), run by tests/zsdec_host
as the wave runs it -- lane 0's work once, the lane sections as loops over 64 lanes -- against libzstd's ZSTD_decompress: frames
libzstd wrote at the archive's levels, mutated frames, and the stand-alone sanitizer program."""
import os
import tempfile

import numpy as np
import pytest

from tests import zsdec_cases as zd
from tests import zstd_cases
from tests.zsdec_host import build as zsdec_build


@pytest.fixture(scope="module")
def decode():
    return zd.host_decoder()


@pytest.fixture(scope="module")
def frames(oracle):
    """[(name, level, input, frame)]: the mixed corpus, the multi-block inputs and the feature inputs at the five levels"""
    inputs = [("corpus%d" % i, d) for i, d in enumerate(zstd_cases.corpus(oracle, 11, 24))]
    inputs += zd.multi_block_inputs(oracle) + zd.feature_inputs()
    return [(name, lv, d, zstd_cases.ref_frame(d, lv)) for name, d in inputs for lv in zd.LEVELS]


@pytest.fixture(scope="module")
def coverage(frames):
    """the precondition of every comparison below: the frames contain every shape the decoder has code for"""
    seen = set()
    for _name, _lv, _d, fr in frames:
        seen |= zd.walk(fr)
    missing = [f for f in zd.REQUIRED if f not in seen]
    assert not missing, missing
    # (the three encodings of the sequence count; the 3-byte one is what "many_sequences" is for: 32 768 sequences in a block)
    assert {"seq_count1", "seq_count2", "seq_count3"} <= seen
    assert {"lit_size_format1", "lit_size_format2", "lit_size_format3", "lit_csize_format3", "lit_csize_format4", "lit_csize_format5"} <= seen
    assert {"fcs1", "fcs2", "fcs4"} <= seen
    return seen


def test_frames_of_libzstd_decode_to_libzstd_s_bytes(decode, frames, coverage):
    assert len(frames) >= 250
    for name, lv, d, fr in frames:
        want = zd.ref_decode(fr, len(d))
        assert want == d, (name, lv)
        st, got = decode(fr)
        assert st == 0, (name, lv, st)
        assert got == want, (name, lv)


def _mutations(frames, seed, per_frame):
    rng = np.random.default_rng(seed)
    for name, lv, d, fr in frames:
        if len(fr) > 60000 and lv != 3:
            continue  # (the long frames at one level: the headers are what differs between levels)
        for p in range(min(len(fr), 24)):  # every position of the headers in front
            m = bytearray(fr)
            m[p] ^= int(rng.integers(1, 256))
            yield name, lv, bytes(m)
        for _ in range(per_frame):
            yield name, lv, zd.mutate(rng, fr)


def test_mutated_frames_never_decode_to_other_bytes_than_libzstd_s(decode, frames, coverage):
    """a status or the bytes: whenever this decoder and libzstd both accept an input, the bytes are equal"""
    both = neither = only_zstd = only_ours = 0
    for name, lv, m in _mutations(frames, 2024, 12):
        st, got = decode(m)
        assert st in (zd.OK, zd.UNSUPPORTED, zd.MALFORMED)
        hdr = m[:18]
        cap = len(got) if st == 0 else 1 << 20
        want = zd.ref_decode(m, cap)
        if st == 0 and want is not None:
            both += 1
            assert got == want, (name, lv, hdr.hex())
        elif st == 0:
            only_ours += 1
        elif want is not None:
            only_zstd += 1
        else:
            neither += 1
    print(f"mutated inputs: {both} accepted by both, {neither} by neither, {only_zstd} by libzstd alone, {only_ours} by this decoder alone")
    assert both > 100 and neither > 100


def test_refused_headers(decode):
    fr = zstd_cases.ref_frame(b"hello hello hello hello", 3)
    assert decode(fr) == (0, b"hello hello hello hello")
    assert decode(b"")[0] == zd.MALFORMED and decode(fr[:3])[0] == zd.MALFORMED
    assert decode(b"\x00" + fr[1:])[0] == zd.MALFORMED                              # wrong magic
    assert decode(b"\x50\x2a\x4d\x18\x04\x00\x00\x00abcd")[0] == zd.UNSUPPORTED     # a skippable frame
    assert decode(fr[:4] + bytes([fr[4] | 0x08]) + fr[5:])[0] == zd.MALFORMED       # the reserved bit
    assert decode(fr[:4] + bytes([fr[4] | 0x04]) + fr[5:] + b"\0\0\0\0")[0] == zd.UNSUPPORTED  # a checksum
    assert decode(fr[:4] + bytes([(fr[4] | 0x01)]) + b"\x07" + fr[5:])[0] == zd.UNSUPPORTED     # a dictionary id
    assert decode(fr[:4] + bytes([(fr[4] | 0x01)]) + b"\x00" + fr[5:]) == (0, b"hello hello hello hello")  # ... of 0: none
    assert decode(fr[:4] + bytes([fr[4] & ~0x20 & 0xFF]) + b"\x00" + fr[6:])[0] == zd.UNSUPPORTED  # a window, no content size
    assert decode(fr[:4] + bytes([0xE0]) + (1 << 31).to_bytes(8, "little") + fr[6:])[0] == zd.UNSUPPORTED  # 2^31 bytes
    assert decode(fr + b"\x00")[0] == zd.MALFORMED                                   # a byte behind the last block
    assert decode(fr[:-1])[0] == zd.MALFORMED


def test_sanitizer_program_runs_clean():
    """the harness as a stand-alone program under -fsanitize=address,undefined, a child process: frames of libzstd's and mutated
    ones, every buffer a heap block of its exact size"""
    out = zsdec_build.run_selftest(seed=3, rounds=40)
    assert out.returncode == 0 and out.stdout.startswith("ok "), out.stdout + out.stderr
    print(out.stdout.strip())


def test_dump_of_the_sanitizer_program_reads_back():
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, "dump.bin")
        out = zsdec_build.run_selftest(seed=5, rounds=3, dump=path)
        assert out.returncode == 0, out.stdout + out.stderr
        items = zsdec_build.read_dump(path)
        assert len(items) > 100 and any(st == 0 for _f, st in items) and any(st == 2 for _f, st in items)
