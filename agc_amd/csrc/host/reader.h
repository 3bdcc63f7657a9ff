// reader.h -- read side of the .agc v3 archive: the CAGCFile interface of the reference
// (src/lib-cxx/agc-api.h:24-100) on top of a plain host decoder.  Used to verify round trips of the
// archives the create path writes and to offer the lib-cxx / py_agc_api surface; decoding is host code
// (zstd + LZ-diff decode + reverse complement + k-overlap stitching,
// src/common/agc_decompressor_lib.cpp:172-286, src/common/segment.cpp:136-400, src/common/lz_diff.cpp:801-836).
#pragma once
#include <cstdint>
#include <cstdio>
#include <memory>
#include <string>
#include <vector>

namespace agc {

// What a device needs to write a sample's FASTA text without this reader's decode loop (GetSamplePlan): the contigs in archive
// order, every segment's source and length, the bytes the sources name cut out of the decoded packs, and the references of the
// groups the sample touches.  Everything behind zstd is left to the caller.
struct SamplePlan {
    enum Kind : uint32_t { RAW = 0, REF = 1, DELTA = 2 }; // a raw group's symbols; a group's reference as it is; a delta against it
    std::vector<uint8_t> names;     // the contig names back to back
    std::vector<uint64_t> name_off; // n_ctg + 1
    std::vector<uint64_t> ctg_seg;  // n_ctg + 1: contig c = segments [ctg_seg[c], ctg_seg[c + 1])
    // per segment (length: its symbols as decode_contig gets them, the overlap included; off / n_bytes: RAW, DELTA -- its bytes in `bytes`)
    std::vector<uint32_t> group_id, in_group_id, rc, length, kind, n_bytes;
    std::vector<uint64_t> off;
    std::vector<uint8_t> bytes;     // every DELTA's delta, every RAW's symbols
    std::vector<uint32_t> groups;   // the distinct groups >= 16 the sample needs, ascending
    std::vector<uint64_t> ref_off;  // groups.size() + 1: group i's reference symbols = ref_bytes[ref_off[i], ref_off[i + 1])
    std::vector<uint8_t> ref_bytes;
};

// What a device needs to write a sample's FASTA text from the archive's own bytes (GetSampleParts): the contigs and segments of
// SamplePlan, and the distinct stored parts the sample touches, as they are stored -- nothing is decoded, no cache is filled.
struct SampleParts {
    enum Coding : uint32_t { STORED = 0, ZSTD = 1 };                // archive metadata 0: the bytes as they are; otherwise one zstd frame
    enum Content : uint32_t { PACK = 0, REF_BYTES = 1, REF_TUPLES = 2 }; // sequences each followed by 0xFF; a reference as symbol bytes; as tuples
    std::vector<uint8_t> names;
    std::vector<uint64_t> name_off, ctg_seg; // as in SamplePlan
    // per segment; length: the collection's raw_length; part / index: RAW, DELTA -- sequence `index` of the pack parts[part]
    std::vector<uint32_t> group_id, in_group_id, rc, length, kind, part, index;
    // per part: its bytes are src[off, off + n_bytes) -- a zstd part without the marker byte behind its frame; group: the stream's group;
    // no: a pack's number in its stream (0 for a reference).  The references come first, ascending by group, then the packs
    std::vector<uint64_t> part_off;
    std::vector<uint32_t> part_bytes, part_coding, part_content, part_group, part_no;
    const uint8_t *src = nullptr; // the archive's bytes (mapped where that is possible): valid until the file is closed
    uint64_t src_bytes = 0;
};

// One query of a batch of contig ranges (GetRangeParts): contig `name` of `sample` (empty: the name must be unique in the archive),
// positions [from, to] inclusive, read by GetCtgSeq's rules.
struct RangeQuery {
    std::string sample, name;
    int64_t from, to;
};

// What a device needs to fetch a batch of contig ranges from the archive's own bytes (GetRangeParts): per query the windows of the
// segments it touches, and the distinct stored parts of the whole batch as SampleParts lists them.
struct RangeParts {
    std::vector<uint64_t> q_seg; // n_q + 1: query q owns the window entries [q_seg[q], q_seg[q + 1])
    std::vector<uint64_t> q_len; // n_q: the symbols query q yields (0: a range at or behind the contig's end)
    // per window entry: the segment as SampleParts has it, and the window [win_from, win_from + win_len) of its ORIENTED symbols
    // (win_len >= 1; behind a contig's first segment win_from >= k: the overlap is accounted for).  A query's windows back to back
    // are its symbols
    std::vector<uint32_t> group_id, in_group_id, rc, length, kind, part, index, win_from, win_len;
    // per part, as in SampleParts: the new references ascending by group, then the packs
    std::vector<uint64_t> part_off;
    std::vector<uint32_t> part_bytes, part_coding, part_content, part_group, part_no;
    const uint8_t *src = nullptr;
    uint64_t src_bytes = 0;
};

class CAGCFile {
    struct Impl;
    std::unique_ptr<Impl> p;

public:
    CAGCFile();
    ~CAGCFile();
    bool Open(const std::string &file_name, bool prefetching = true);
    bool Close();
    // contig length, or < 0 for errors (-1 unknown, -2 name not unique and sample empty)
    int64_t GetCtgLen(const std::string &sample, const std::string &name) const;
    // [start, end] inclusive as in the reference (start = end = -1: whole contig); returns 0 or < 0
    int GetCtgSeq(const std::string &sample, const std::string &name, int64_t start, int64_t end, std::string &buffer) const;
    int NSample() const;
    int NCtg(const std::string &sample) const;
    int ListSample(std::vector<std::string> &samples) const; // sorted, as the reference
    int ListSampleStored(std::vector<std::string> &samples) const; // archive order (get_samples_list(v, false), used by getcol)
    int GetReferenceSample(std::string &sample) const;
    int ListCtg(const std::string &sample, std::vector<std::string> &names) const;
    // compression parameters stored in the archive: k, min_match_len, pack_cardinality, segment_size
    bool GetParams(uint32_t &k, uint32_t &mml, uint32_t &pack, uint32_t &segment_size) const;
    // key -> value pairs of the file_type_info stream (agc info -v 1)
    bool GetFileTypeInfo(std::vector<std::pair<std::string, std::string>> &info) const;
    // whole sample as FASTA text (agc getset): ">name\n" + 80-column lines
    bool GetSampleFasta(const std::string &sample, std::string &out, uint32_t line_length = 80) const;
    // all contigs of a sample as symbol codes (GetSampleSequences, agc_decompressor_lib.cpp; used by append -a)
    bool GetSampleCodes(const std::string &sample, std::vector<std::string> &names, std::vector<std::vector<uint8_t>> &codes) const;
    // the same, written contig by contig to an open stream (what the CLI uses: no sample-size string is built)
    bool WriteSampleFasta(const std::string &sample, FILE *f, uint32_t line_length = 80) const;
    // the plan of a whole sample (see SamplePlan); false: unknown sample or an unreadable part
    bool GetSamplePlan(const std::string &sample, SamplePlan &plan) const;
    // the stored parts of a whole sample (see SampleParts): pack idx / pack_cardinality of x<group>d for every RAW and DELTA segment,
    // part 0 of x<group>r for every group >= 16 the sample touches that is not among have_groups; false: unknown sample, a part the
    // archive does not hold
    bool GetSampleParts(const std::string &sample, const uint32_t *have_groups, size_t n_have, SampleParts &parts) const;
    // the windows and stored parts of a batch of contig ranges (see RangeParts; the arithmetic: ../range_plan.h); nothing is
    // decompressed, no cache is touched.  false: an unknown or ambiguous contig -- *bad_query (when given) is the first such query --
    // or a part the archive does not hold (*bad_query = -1)
    bool GetRangeParts(const std::vector<RangeQuery> &queries, const uint32_t *have_groups, size_t n_have, RangeParts &parts, int64_t *bad_query = nullptr) const;
    // one `agc getctg` query -- contig[@sample][:from-to] (agc_decompressor_lib.h:127-130) -- as FASTA text;
    // the header is the full contig name (+ ":from-to" when a range was given), core/agc_decompressor.cpp:478-567
    bool GetContigFasta(const std::string &query, std::string &out, uint32_t line_length, std::string &err) const;
};

} // namespace agc
