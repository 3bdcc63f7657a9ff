"""The read side on fuzz archives: the cases, and what tests/test_read_fuzz_cpu.py (the CPU restatements of the reader's plans) and
tests/test_gpu_read_fuzz.py (agc_amd/devread.py: DeviceReader against the host reader) share.  The collections are those of
tests/fuzz.py: parameters, contig edits, -c, -a and create/append splits drawn from one seed.  No GPU in here."""
import os

import numpy as np

from tests import fuzz
from tests import ranges_cases as RC

# (seed, kwargs of fuzz.make_case).  Together: every k of fuzz.make_case, min-match-lengths 15 .. 32, segment sizes 100 .. 60000,
# batch sizes 1 .. 50, -c, -a and both, plans of one, two and three steps, contigs shorter than k, a contig name twice in a sample,
# lower case.  -b is the pack cardinality, so the cases with -b 1 .. 5 have groups of several packs already; of the two `many`
# cases (20 - 70 samples) 8 is the smallest by input bytes among the seeds 0 .. 39 with a second pack in a group (-b 1: every
# segment a pack of its own), 206 the smallest among 0 .. 259 that has one at the default cardinality of 50 (none of 0 .. 39 has).
# tests/test_read_fuzz_cpu.py: test_the_cases_cover_the_read_path asserts what the list must supply (and prints this table)
#
#   case      k  l  s     b  flags  steps    kinds x rc (R raw, F ref, D delta; +/-)  part shapes        max part_no  max segs  samples
#   3         31 16 100   50 -a     [5,3]    R+ F+ F- D+ D-                           sp sr zp zr zt     0            102       8
#   9         21 21 100   5  -      [3]      R+ F+ F- D+                              sp sr zp zt        0            1403      2
#   11        17 15 1000  5  -c -a  [3,3,1]  R+ F+ F- D+ D-                           sp sr zp zt        1            102       25
#   22        31 21 60000 1  -      [1,5,3]  R+ F+ F- D+ D-                           sp sr zp zt        9            3         9
#   30        17 15 300   1  -      [4,2,2]  R+ F+ F- D+ D-                           sp sr zp zt        8            69        8
#   70        25 20 300   2  -      [7,1]    R+ F+ F- D+ D-                           sp sr zp zt        2            49        8
#   85        31 15 1000  3  -      [8]      R+ F+ F- D+ D-                           sp sr zp zt        2            82        8
#   93        32 32 300   3  -      [3,5]    R+ F+ F- D+ D-                           sp sr zp zt        2            7         8
#   99        32 24 100   3  -      [3,6]    R+ F+ F- D+ D-                           sp sr zp zt        3            102       9
#   100       31 29 100   2  -c     [9]      R+ F+ F- D+ D-                           sp sr zp zt        7            142       54
#   101       19 19 100   5  -a     [3,2,1]  F+ F- D+ D-                              sp sr zp zt        0            1203      6
#   112       19 20 100   5  -c -a  [9]      R+ F+ F- D+ D-                           sp sr zp zr zt     0            10        29
#   1091      25 15 2500  3  -c     [3,1]    R+ F+ F- D+ D-                           sp sr zp zt        0            58        12
#   21201     21 19 100   1  -a     [1,5]    R+ F+ F- D+ D-                           sp sr zp zr zt     5            67        6
#   8-many    31 20 300   1  -      [10,14]  R+ F+ F- D+ D-                           sp sr zp zt        16           6         23
#   206-many  25 24 100   50 -      [28,38]  R+ F+ F- D+ D-                           sp sr zp zt        1            16        66
#   (s / z: stored, zstd; p / r / t: pack, reference as bytes, reference as tuples)
SEEDS = [(s, {}) for s in (3, 9, 11, 22, 30, 70, 85, 93, 99, 100, 101, 112, 1091, 21201)] + [(8, {"many": True}), (206, {"many": True})]
IDS = [f"{s}" + "".join(f"-{k}" for k, v in sorted(kw.items()) if v) for s, kw in SEEDS]


def write(cli, seed, outdir, threads="3", env=None, **kw):
    """the case of `seed` written by `cli` (create and the appends) under outdir -> (the last step's archive, the case, the files of
    all steps)"""
    outdir = str(outdir)
    case = fuzz.make_case(seed, os.path.join(outdir, "in"), **kw)
    got, errs = fuzz.run_case(cli, case, outdir, "rf", threads=threads, env=env)
    assert None not in got and len(got) == len(case["steps"]) and all(got), f"seed {seed}: a step died: " + errs[-1][-1000:]
    return os.path.join(outdir, f"rf_{len(got) - 1}.agc"), case, case["files"]


def short_name(name):
    """up to the first white space (agc_amd/csrc/host/archive_read.h: short_name)"""
    for i, ch in enumerate(name):
        if ch in " \n\r\t":
            return name[:i]
    return name


def addressable(names):
    """the contigs of one sample that their own name finds: the reader resolves a name to the FIRST contig with its short name
    (reader.cpp: find_contig, as the reference's get_contig_desc does), so a later copy of a repeated name is reached by no query ->
    the indices, ascending"""
    first = {}
    for c, n in enumerate(names):
        first.setdefault(short_name(n), c)
    return sorted(first.values())


def coverage(reader, path):
    """what the archive supplies to the read path, from GetParams, GetSamplePlan, GetSampleParts and GetRangeParts (the whole of every
    addressable contig)"""
    a = reader.CAGCFile()
    assert a.Open(path)
    prm = a.GetParams()
    k = prm["k"]
    cov = {"k": k, "min_match_len": prm["min_match_len"], "segment_size": prm["segment_size"], "pack_cardinality": prm["pack_cardinality"], "kinds": set(), "shapes": set(), "max_part_no": 0,
           "short_contig": False, "empty_contig": False, "repeated_name": False, "max_segments": 0, "n_samples": 0}
    for s in a.ListSample():
        cov["n_samples"] += 1
        plan, parts = a.GetSamplePlan(s), a.GetSampleParts(s)
        names = a.ListCtg(s)
        cov["repeated_name"] |= len(set(names)) < len(names)
        cov["kinds"] |= set(zip(plan["kind"].tolist(), plan["rc"].tolist()))
        cs = plan["ctg_seg"].astype(np.int64)
        for c in range(cs.size - 1):  # (the later copy of a repeated name may be a contig of no segments)
            n_seg = int(cs[c + 1] - cs[c])
            cov["empty_contig"] |= n_seg == 0
            cov["short_contig"] |= 0 < int(plan["length"][cs[c]:cs[c + 1]].sum()) - k * (n_seg - 1) < k
            cov["max_segments"] = max(cov["max_segments"], n_seg)
        r = a.GetRangeParts([(s, names[c], -1, -1) for c in addressable(names)])
        for p in (parts, r):
            cov["shapes"] |= set(zip(p["part_coding"].tolist(), p["part_content"].tolist()))
            pack = p["part_content"] == reader.PART_PACK
            cov["max_part_no"] = max([cov["max_part_no"]] + p["part_no"][pack].tolist())
    assert a.Close()
    return cov


def queries(host, seed):
    """a range inside the first segment of every kind and orientation, the boundary ranges of three contigs (those with the most
    segments), 200 seeded random ranges of 1 - 3 000 symbols across all samples -> (queries, the (kind, rc) pairs the batch has a
    window in, those the archive has in segments that keep a symbol).  Only contigs that their name finds (addressable)"""
    k = host.GetParams()["k"]
    ctgs, in_archive, out = [], set(), []
    for s in host.ListSample():
        plan = host.GetSamplePlan(s)
        names = host.ListCtg(s)
        for c in addressable(names):
            name = names[c]
            lo, hi = int(plan["ctg_seg"][c]), int(plan["ctg_seg"][c + 1])
            lens = plan["length"][lo:hi].tolist()
            ctgs.append((len(lens), s, name, lens, sum(lens) - k * (len(lens) - 1)))
            pos = 0
            for i, n in enumerate(lens):  # the first segment of every kind and orientation that keeps a symbol: a range inside it
                kept = n - (k if i else 0)
                pair = (int(plan["kind"][lo + i]), int(plan["rc"][lo + i]))
                if kept > 0 and pair not in in_archive:
                    in_archive.add(pair)
                    out.append((s, name, pos + kept // 3, pos + kept - 1 - kept // 3))
                pos += kept
    for _n, s, name, lens, _len in sorted(ctgs, key=lambda x: -x[0])[:3]:
        out += [(s, name, f, t) for f, t in RC.contig_ranges(lens, k)]
    rng = np.random.default_rng(seed)
    for _ in range(200):
        _n, s, name, _lens, n = ctgs[int(rng.integers(len(ctgs)))]
        f = int(rng.integers(max(n, 1)))
        out.append((s, name, f, f + int(rng.integers(1, 3001)) - 1))
    p = host.GetRangeParts(out)
    return out, set(zip(p["kind"].tolist(), p["rc"].tolist())), in_archive
