"""CPU: the read side on the fuzz archives of tests/readfuzz_cases.py, written through the device stand-in (tests/devsim).  Per case the
host reader gives back the input contigs (fuzz.archive_round_trips: no plan involved), and the three restatements of the reader's
plans hold -- the sample plan (test_read_plan_cpu.check_archive), the stored parts, every zstd frame through the CPU build of the
GPU's decoder (test_read_parts_cpu.check_archive), and the windows of contig ranges (test_range_parts_cpu.check_archive).  One more
test states what the cases together must supply to the read path: tests/test_gpu_read_fuzz.py reads the same cases on the device."""
import pytest

from tests import fuzz
from tests import readfuzz_cases as RF
from tests import test_range_parts_cpu as RANGES
from tests import test_read_parts_cpu as PARTS
from tests import test_read_plan_cpu as PLAN
from tests.test_read_parts_cpu import gpu_decoder  # noqa: F401  (fixtures)
from tests.test_read_plan_cpu import rd  # noqa: F401


@pytest.fixture(scope="module")
def archives(tmp_path_factory):
    """i -> (archive, case, files) of RF.SEEDS[i], written once"""
    from tests.devsim import build as simbuild
    cli, done = simbuild.build(), {}

    def get(i):
        if i not in done:
            seed, kw = RF.SEEDS[i]
            done[i] = RF.write(cli, seed, tmp_path_factory.mktemp(f"readfuzz_{RF.IDS[i]}"), **kw)
        return done[i]
    return get


@pytest.mark.parametrize("i", range(len(RF.SEEDS)), ids=RF.IDS)
def test_the_host_reader_gives_back_the_input(archives, i):
    path, _case, files = archives(i)
    assert fuzz.archive_round_trips(path, files)


@pytest.mark.parametrize("i", range(len(RF.SEEDS)), ids=RF.IDS)
def test_sample_plans(rd, oracle, archives, i):  # noqa: F811
    PLAN.check_archive(rd, oracle, archives(i)[0])


@pytest.mark.parametrize("i", range(len(RF.SEEDS)), ids=RF.IDS)
def test_sample_parts(rd, gpu_decoder, archives, i):  # noqa: F811
    PARTS.check_archive(rd, archives(i)[0], gpu_decoder)


@pytest.mark.parametrize("i", range(len(RF.SEEDS)), ids=RF.IDS)
def test_range_parts(rd, oracle, archives, i):  # noqa: F811
    RANGES.check_archive(rd, oracle, archives(i)[0])


def test_the_cases_cover_the_read_path(rd, archives):  # noqa: F811
    """conditions on the inputs: where one fails a seed of RF.SEEDS is replaced, the condition stays"""
    cov, flags, steps = [], set(), set()
    for i in range(len(RF.SEEDS)):
        path, case, _files = archives(i)
        cov.append(RF.coverage(rd, path))
        flags.add(tuple(case["carry"]))
        steps.add(len(case["steps"]))
        a = case["args"]
        print(RF.IDS[i], "k", a[1], "l", a[3], "s", a[5], "b", a[7], " ".join(case["carry"]) or "-", "steps", case["steps"], "kinds x rc", sorted(cov[-1]["kinds"]),
              "shapes", sorted(cov[-1]["shapes"]), "max part_no", cov[-1]["max_part_no"], "max segments", cov[-1]["max_segments"], "samples", cov[-1]["n_samples"])
    assert {c["k"] for c in cov} == {17, 19, 21, 25, 31, 32}
    assert {15, 32} <= {c["min_match_len"] for c in cov}
    # every kind in either orientation an archive can hold: a segment without a terminal splitter is stored as it was read (no
    # fallback minimizers: the writer has no k-mer to orient it by), so (RAW, rc = 1) is in no archive, whatever the seed -- the
    # kernels see it in the handmade plans of tests/fastaout_cases.py alone
    assert set().union(*(c["kinds"] for c in cov)) == {(rd.PLAN_RAW, 0), (rd.PLAN_REF, 0), (rd.PLAN_REF, 1), (rd.PLAN_DELTA, 0), (rd.PLAN_DELTA, 1)}
    # every part shape an archive can hold: a reference stored as it is (metadata 0) has no marker byte and is symbol bytes by
    # definition (reader.cpp: GetSampleParts), so there is no (STORED, REF_TUPLES); the stored references are REF_BYTES
    assert set().union(*(c["shapes"] for c in cov)) == {(rd.PART_STORED, rd.PART_PACK), (rd.PART_ZSTD, rd.PART_PACK), (rd.PART_ZSTD, rd.PART_REF_TUPLES),
                                                        (rd.PART_STORED, rd.PART_REF_BYTES), (rd.PART_ZSTD, rd.PART_REF_BYTES)}
    assert any(c["max_part_no"] >= 1 for c in cov)
    # ... and at the default cardinality, where the in-group id splits into a pack number AND an index inside the pack
    assert any(c["max_part_no"] >= 1 and c["pack_cardinality"] == 50 for c in cov)
    assert any(c["short_contig"] for c in cov)
    assert any(c["repeated_name"] for c in cov)
    assert {("-c",), ("-a",), ("-c", "-a")} <= flags and 3 in steps
    assert any(c["max_segments"] >= 100 for c in cov)
