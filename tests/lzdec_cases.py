"""Handcrafted LZ-diff deltas for the decode tests (tests/test_lz_decode_host.py on the CPU, tests/test_gpu_lz_decode.py on the
GPU): the smallest shapes at which a decode in 64-byte strips can still go wrong, and the malformed deltas it must reject."""
import numpy as np

MML = 20
STATUS_OK, BAD_TOKEN, BAD_LITERAL_REF, BAD_MATCH, TOO_LONG = range(5)  # agc_amd/csrc/lz_decode.h: Status


class Delta:
    """writes tokens and keeps pred_pos as the decoder will, so that a match can be asked for by its reference position"""

    def __init__(self, ref_size, mml=MML):
        self.b, self.pred, self.ref_size, self.mml = bytearray(), 0, ref_size, mml

    def lit(self, *codes):
        for c in codes:
            self.b.append(ord("A") + c)
            self.pred += 1
        return self

    def bang(self):
        self.b += b"!"
        self.pred += 1
        return self

    def nrun(self, n):
        self.b += bytes([30]) + str(n - 4).encode() + bytes([4])
        return self

    def match(self, ref_pos, n=None):
        self.b += str(ref_pos - self.pred).encode()
        if n is not None:
            self.b += b"," + str(n - self.mml).encode()
        self.b += b"."
        self.pred = self.ref_size if n is None else ref_pos + n
        return self

    def pad_to(self, size):
        """literals up to `size` bytes"""
        while len(self.b) < size:
            self.lit(len(self.b) % 21)
        assert len(self.b) == size
        return self

    def raw(self, data):
        self.b += data
        return self

    def bytes(self):
        return np.frombuffer(bytes(self.b), np.uint8).copy()


def references():
    rng = np.random.default_rng(11)
    clean = rng.integers(0, 4, 4000).astype(np.uint8)
    esc = rng.integers(0, 4, 2500).astype(np.uint8)
    esc[1030] = 4  # block 1 (1024 .. 2047) is escaped, blocks 0 and 2 are clean
    return {"clean": clean, "esc": esc}


def valid_cases():
    """-> [(name, reference name, delta bytes)]"""
    out = []
    C, E = 4000, 2500
    for n in (0, 1, 63, 64, 65, 128, 129):
        out.append((f"literals_{n}_bytes", "clean", Delta(C).pad_to(n)))
    # a match token over the strip boundary: bytes 62.. "12|34,5.", 61.. "12,|5.", 62.. "12|,5.", 60.. "12,5|."
    out.append(("straddle_diff_digits", "clean", Delta(C).pad_to(62).match(62 + 1234, MML + 5).lit(1, 2)))
    out.append(("straddle_after_comma", "clean", Delta(C).pad_to(61).match(61 + 12, MML + 5).lit(1, 2)))
    out.append(("straddle_before_comma", "clean", Delta(C).pad_to(62).match(62 + 12, MML + 5).lit(1, 2)))
    out.append(("dot_is_byte_64", "clean", Delta(C).pad_to(60).match(60 + 12, MML + 5).lit(1, 2).bang()))
    out.append(("dot_is_byte_63", "clean", Delta(C).pad_to(59).match(59 + 12, MML + 5).lit(1, 2).bang()))
    d = Delta(C).pad_to(61).nrun(14).lit(3).bang()
    assert d.b[64] == 4 and d.b[61] == 30
    out.append(("nrun_terminator_is_byte_64", "clean", d))
    out.append(("diff_zero_negative_widest", "clean",
                Delta(C).match(0, 30).match(30, 25).match(3, 40).match(C - 25, 25).match(0, 33).lit(4)))
    out.append(("match_to_end_last", "clean", Delta(C).lit(0, 1).match(3900)))
    out.append(("match_to_end_in_the_middle", "clean", Delta(C).lit(0, 1).match(3950).lit(2, 3, 20).nrun(4).lit(0)))
    out.append(("match_to_end_of_nothing", "clean", Delta(C).match(C).lit(1)))
    out.append(("bang_after_match_and_nrun", "clean", Delta(C).match(100, 21).bang().nrun(7).bang().bang().lit(5)))
    out.append(("literal_codes_0_20", "clean", Delta(C).lit(*range(21))))
    out.append(("escaped_reference", "esc",
                Delta(E).match(1008, 40).bang().match(1025, 21).match(2033, 50).match(1030 - 3, MML).match(1039, 1100)
                .match(1030, MML).bang().match(2479)))
    out.append(("escaped_reference_ends_at_ref_size", "esc", Delta(E).match(2047, E - 2047).lit(7).match(1030)))
    out.append(("long_output", "clean", Delta(C).lit(1).match(5, 3 * 64 * 16 + 77).bang()))
    out.append(("nrun_long", "clean", Delta(C).nrun(4).nrun(64).nrun(1000).lit(2)))
    return [(name, ref, d.bytes()) for name, ref, d in out]


def rejected_cases():
    """-> [(name, reference name, delta bytes, status)]: every one must be refused, none may be decoded"""
    C = 4000
    out = [
        ("truncated_match", Delta(C).lit(1).raw(b"12,5"), BAD_TOKEN),
        ("truncated_match_no_length", Delta(C).lit(1).raw(b"12"), BAD_TOKEN),
        ("truncated_match_at_comma", Delta(C).pad_to(63).raw(b"12,"), BAD_TOKEN),
        ("truncated_nrun", Delta(C).lit(1).raw(bytes([30]) + b"12"), BAD_TOKEN),
        ("nrun_starter_alone", Delta(C).lit(1).raw(bytes([30])), BAD_TOKEN),
        ("nrun_closed_by_dot", Delta(C).raw(bytes([30]) + b"12.").lit(1), BAD_TOKEN),
        ("eleven_digits", Delta(C).raw(b"12345678901,5.").lit(1), BAD_TOKEN),
        ("eleven_digits_of_length", Delta(C).raw(b"1,12345678901.").lit(1), BAD_TOKEN),
        ("stray_byte", Delta(C).lit(1).raw(b"Z").lit(2), BAD_TOKEN),
        ("literal_inside_a_number", Delta(C).raw(b"12A,5.").lit(2), BAD_TOKEN),
        ("match_one_past_the_end", Delta(C).match(C - MML - 4, MML + 5).lit(1), BAD_MATCH),
        ("match_starts_past_the_end", Delta(C).match(C + 1), BAD_MATCH),
        ("bang_at_ref_size", Delta(C).lit(1).match(3990).bang(), BAD_LITERAL_REF),
        ("bang_past_ref_size", Delta(C).match(3990).lit(1, 2).bang(), BAD_LITERAL_REF),
        ("negative_ref_pos", Delta(C).lit(1, 2).raw(b"-3,5.").lit(1), BAD_MATCH),
        ("negative_ref_pos_to_end", Delta(C).raw(b"-1."), BAD_MATCH),
        ("bad_token_in_the_third_strip", Delta(C).pad_to(130).raw(b"-140,5.").lit(1), BAD_MATCH),
        ("two_to_the_32_symbols", Delta(C).raw(bytes([30]) + str(2 ** 32 - 4).encode() + bytes([4])), TOO_LONG),
    ]
    return [(name, "clean", d.bytes(), st) for name, d, st in out]
