"""CPU: agc_amd/csrc/parts_unpack.h compiled for the host (tests/partsunpack_host) and run in the kernels' order -- a wave is a loop
over 64 lanes, a ballot a loop over their bits, a launch a loop over 16-byte chunks -- against the plain numpy restatements of
tests/partsunpack_cases.py, on the shapes tests/test_gpu_sample_parts.py sends through the device; and the stand-alone sanitizer
program."""
import ctypes as C

import numpy as np
import pytest

from tests import partsunpack_cases as PC
from tests.partsunpack_host import build as pubuild

u8p, u32p, u64p = C.POINTER(C.c_uint8), C.POINTER(C.c_uint32), C.POINTER(C.c_uint64)
GUARD = 0xABABABAB


@pytest.fixture(scope="module")
def pu():
    L = C.CDLL(pubuild.build())
    L.pu_pack_index.argtypes = [C.c_char_p, C.c_uint32, C.c_uint32, u32p]
    L.pu_pack_index.restype = C.c_uint32
    L.pu_tuple_shape.argtypes = [C.c_uint64, C.c_uint32, u32p, u64p]
    L.pu_tuple_shape.restype = C.c_uint32
    L.pu_tuples_unpack.argtypes = [C.c_char_p, C.c_uint64, C.c_uint32, u8p, C.c_uint64, u64p]
    L.pu_tuples_unpack.restype = C.c_uint32
    return L


def index(pu, pack, seq_cap):
    """-> (count, the row of seq_cap end offsets with 8 guard words behind it)"""
    row = np.full(seq_cap + 8, GUARD, np.uint32)
    return pu.pu_pack_index(bytes(pack), len(pack), seq_cap, row.ctypes.data_as(u32p)), row


def check_pack(pu, pack, seq_cap):
    want = PC.pack_ends(pack)
    count, row = index(pu, pack, seq_cap)
    kept = min(want.size, seq_cap)
    assert count == want.size  # exact, also above the cap
    assert np.array_equal(row[:kept], want[:kept])
    assert (row[kept:] == GUARD).all()  # nothing behind the sequences there are, nothing past the cap


@pytest.mark.parametrize("name,pack", PC.pack_shapes(), ids=[n for n, _p in PC.pack_shapes()])
def test_pack_shapes(pu, name, pack):
    for seq_cap in (0, 1, 2, 50, 200):
        check_pack(pu, pack, seq_cap)
    # the restatement itself: the sequences put back together are the pack up to its last terminator
    seqs = PC.pack_sequences(pack)
    assert PC.pack_of(seqs) == pack[:len(PC.pack_of(seqs))] and b"\xff" not in pack[len(PC.pack_of(seqs)):]


@pytest.mark.parametrize("seq_cap", [1, 50])
def test_exactly_the_cap_and_one_more(pu, seq_cap):
    for _name, pack in PC.capped_packs(seq_cap):
        n = len(PC.pack_sequences(pack))
        assert n in (seq_cap, seq_cap + 1)
        check_pack(pu, pack, seq_cap)
        count, row = index(pu, pack, seq_cap)
        assert count == n and (row[seq_cap:] == GUARD).all() and (row[:seq_cap] != GUARD).all()


def unpack(pu, t, a, cap):
    out = np.full(cap + 16, 0xAA, np.uint8)
    n = C.c_uint64(0)
    st = pu.pu_tuples_unpack(bytes(t), len(t), a, out.ctypes.data_as(u8p), cap, C.byref(n))
    return st, n.value, out


@pytest.mark.parametrize("name,t,sym", PC.tuple_shapes(), ids=[n for n, _t, _s in PC.tuple_shapes()])
def test_tuple_shapes(pu, name, t, sym):
    nb, n = C.c_uint32(9), C.c_uint64(9)
    assert pu.pu_tuple_shape(len(t), t[-1], C.byref(nb), C.byref(n)) == PC.OK and n.value == sym.size
    assert nb.value == (t[-1] >> 4 if t[-1] >> 4 in (2, 3, 4) else 0)
    for a in (0, 1, 7, 15):  # the output's first byte at these addresses modulo 16: every chunk's range moves
        st, got_n, out = unpack(pu, t, a, sym.size)
        assert (st, got_n) == (PC.OK, sym.size)
        assert np.array_equal(out[:sym.size], sym) and (out[sym.size:] == 0xAA).all(), a


@pytest.mark.parametrize("name,t", PC.refused_tuples(), ids=[n for n, _t in PC.refused_tuples()])
def test_refused_tuples_are_left_unwritten(pu, name, t):
    assert PC.symbols_of(t) is None
    st, _n, out = unpack(pu, t, 3, 64)
    assert st == PC.BAD_TUPLES and (out == 0xAA).all()


def test_sanitizer_program_runs_clean():
    """the harness as a stand-alone program under -fsanitize=address,undefined, a child process: seeded random packs and tuple
    streams, a third of the streams malformed, every buffer a heap block of its exact size"""
    out = pubuild.run_selftest(seed=7, rounds=4000)
    assert out.returncode == 0 and out.stdout.startswith("ok 4000 rounds"), out.stdout + out.stderr
    refused = int(out.stdout.split(",")[1].split()[0])
    assert 1100 < refused < 1600  # a third of them
