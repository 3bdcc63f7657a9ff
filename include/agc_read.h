/* agc_read.h -- C ABI of the read side, library libagc_read.so.
 *
 * Same entry points, argument meaning and return values as the C section of the reference's
 * src/lib-cxx/agc-api.h:118-213 (implementation src/lib-cxx/lib-cxx.cpp:123-330), so a program written
 * against the reference's libagc links against this library unchanged.  Host code only: decoding an archive
 * (zstd + LZ-diff decode + reverse complement + stitching) is not part of the GPU hot path.
 * Two additions, marked "extension", return FASTA text the way `agc getset` / `agc getctg` write it; a third hands out the
 * PLAN of a sample -- what is left to do behind zstd -- for a caller that assembles the text elsewhere (agc_amd/devread.py: on
 * the GPU, include/agc_hip.h: agc_hip_sample_fasta); a fourth hands out the stored PARTS the sample touches, undecoded, for a caller
 * that also decodes elsewhere (agc_hip_sample_fasta_parts).  This library itself stays host code.
 */
#ifndef AGC_READ_H
#define AGC_READ_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct agc_t agc_t;

/* agc-api.h:118  NULL for error; prefetching is accepted and ignored (the file is always mapped whole) */
agc_t *agc_open(char *fn, int prefetching);
/* agc-api.h:125  0 for success, -1 for error; frees the handle */
int agc_close(agc_t *agc);
/* agc-api.h:138  contig length or < 0 (-1 unknown, -2 name not unique and sample NULL) */
int agc_get_ctg_len(const agc_t *agc, const char *sample, const char *name);
/* agc-api.h:150  [start, end] inclusive; buf must hold end - start + 2 bytes; returns the length written or < 0 */
int agc_get_ctg_seq(const agc_t *agc, const char *sample, const char *name, int start, int end, char *buf);
/* agc-api.h:157 */
int agc_n_sample(const agc_t *agc);
/* agc-api.h:165 */
int agc_n_ctg(const agc_t *agc, const char *sample);
/* agc-api.h:172  malloc'ed string, free with agc_string_destroy */
char *agc_reference_sample(const agc_t *agc);
/* agc-api.h:180  NULL-terminated malloc'ed array (sorted sample names), free with agc_list_destroy */
char **agc_list_sample(const agc_t *agc, int *n_sample);
/* agc-api.h:189 */
char **agc_list_ctg(const agc_t *agc, const char *sample, int *n_ctg);
/* agc-api.h:196 */
int agc_list_destroy(char **list);
/* agc-api.h:203 */
int agc_string_destroy(char *sample);

/* extension: whole sample as FASTA text (`agc getset`), malloc'ed, *len = bytes; NULL for error */
char *agc_get_sample_fasta(const agc_t *agc, const char *sample, int line_length, long long *len);
/* extension: k, min_match_len, pack_cardinality, segment_size stored in the archive; 0 for success */
int agc_get_params(const agc_t *agc, unsigned *k, unsigned *min_match_len, unsigned *pack_cardinality, unsigned *segment_size);

/* extension: the plan of a whole sample.  Contig c (archive order) has the name names[name_off[c], name_off[c+1]) and the segments
 * [ctg_seg[c], ctg_seg[c+1]); a segment has its group, its index in the group, its orientation, its length in symbols (the
 * k-symbol overlap with the segment in front included) and a kind: its symbols are bytes[off, off + seg_bytes) as they are
 * (AGC_PLAN_RAW: groups < 16), the reference of its group as it is (AGC_PLAN_REF), or the LZ-diff delta bytes[off, off + seg_bytes)
 * against that reference (AGC_PLAN_DELTA).  groups: the n_groups distinct groups >= 16 the sample needs, ascending; the reference
 * symbols of groups[i] are ref_bytes[ref_off[i], ref_off[i+1]).  The pointers belong to the plan and live until it is destroyed. */
enum { AGC_PLAN_RAW = 0, AGC_PLAN_REF = 1, AGC_PLAN_DELTA = 2 };
typedef struct agc_plan_t agc_plan_t;
typedef struct {
    uint64_t n_ctg, n_seg, n_bytes, n_groups;
    const char *names;
    const uint64_t *name_off; /* n_ctg + 1 */
    const uint64_t *ctg_seg;  /* n_ctg + 1 */
    const uint32_t *group_id, *in_group_id, *rc, *length, *kind, *seg_bytes; /* n_seg each */
    const uint64_t *off;      /* n_seg */
    const uint8_t *bytes;     /* n_bytes */
    const uint32_t *groups;   /* n_groups */
    const uint64_t *ref_off;  /* n_groups + 1 */
    const uint8_t *ref_bytes;
} agc_plan_view;
/* NULL for an unknown sample or an unreadable archive part */
agc_plan_t *agc_get_sample_plan(const agc_t *agc, const char *sample);
/* fills *out; 0 for success */
int agc_plan_fields(const agc_plan_t *plan, agc_plan_view *out);
/* frees the plan (NULL: nothing to do); returns 0 */
int agc_plan_destroy(agc_plan_t *plan);

/* extension: the stored PARTS of a whole sample -- the plan above without its decode, for a caller that decodes elsewhere
 * (agc_amd/devread.py: on the GPU, include/agc_hip.h: agc_hip_sample_fasta_parts).  Contigs, names and the segments' group,
 * index in the group, orientation and kind as in the plan; length is the length the collection stores for the segment; a RAW or
 * DELTA segment is sequence seg_index (counted from 0) of the pack seg_part.  The n_parts distinct parts the sample touches:
 * part 0 of the reference stream of every group >= 16 that is not among have_groups (ascending by group), then pack
 * index / pack_cardinality of the delta stream of every group a RAW or DELTA segment names.  Part i is the bytes
 * src[part_off[i], part_off[i] + part_bytes[i]) of the archive, coded AGC_PART_STORED (as they are) or AGC_PART_ZSTD (one frame; the
 * marker byte the archive keeps behind it is not counted), and holds AGC_PART_PACK (sequences, each followed by 0xFF),
 * AGC_PART_REF_BYTES (a reference, one symbol per byte) or AGC_PART_REF_TUPLES (a reference packed 2-4 symbols per byte, its marker
 * byte last); part_group / part_no: its group and, for a pack, its number in the stream.  Nothing is decompressed and none of the
 * reader's caches is touched.  src belongs to the archive (valid until agc_close), everything else to the parts object. */
enum { AGC_PART_STORED = 0, AGC_PART_ZSTD = 1 };
enum { AGC_PART_PACK = 0, AGC_PART_REF_BYTES = 1, AGC_PART_REF_TUPLES = 2 };
typedef struct agc_parts_t agc_parts_t;
typedef struct {
    uint64_t n_ctg, n_seg, n_parts, src_bytes;
    const uint8_t *src;
    const char *names;
    const uint64_t *name_off; /* n_ctg + 1 */
    const uint64_t *ctg_seg;  /* n_ctg + 1 */
    const uint32_t *group_id, *in_group_id, *rc, *length, *kind, *seg_part, *seg_index; /* n_seg each */
    const uint64_t *part_off;                                                           /* n_parts */
    const uint32_t *part_bytes, *part_coding, *part_content, *part_group, *part_no;     /* n_parts each */
} agc_parts_view;
/* NULL for an unknown sample or a part the archive does not hold */
agc_parts_t *agc_get_sample_parts(const agc_t *agc, const char *sample, const uint32_t *have_groups, uint64_t n_have);
/* fills *out; 0 for success */
int agc_parts_fields(const agc_parts_t *parts, agc_parts_view *out);
/* frees the parts object (NULL: nothing to do); returns 0 */
int agc_parts_destroy(agc_parts_t *parts);

/* extension: the stored parts a BATCH of contig ranges needs, for a caller that decodes elsewhere (agc_amd/devread.py: on the GPU,
 * include/agc_hip.h: agc_hip_ranges_parts).  Query q is contig names[q] of samples[q] -- full or short name; samples NULL, or
 * samples[q] NULL or empty: the name must be unique in the archive -- positions [from[q], to[q]] inclusive, read as agc_get_ctg_seq
 * reads them: from < 0 is 0, to < 0 is the contig's end, from > to is the whole contig, everything is clamped to the contig; a range
 * that starts at or behind the contig's end is a valid query of no symbols.  Query q yields q_len[q] symbols and owns the window
 * entries [q_seg[q], q_seg[q+1]): one per segment that contributes at least one symbol, with the segment's fields as in
 * agc_parts_view and the window [win_from, win_from + win_len) of its ORIENTED symbols (win_len >= 1; the k-symbol overlap is
 * accounted for: behind a contig's first segment win_from >= k).  A query's windows back to back, in entry order, are its symbols.
 * The parts: the distinct parts of the whole batch, each once, in the order and with the fields of agc_get_sample_parts (new
 * references ascending by group -- those of have_groups left out -- then packs).  Nothing is decompressed and none of the reader's
 * caches is touched.  NULL: an unknown or ambiguous contig -- *bad_query (may be NULL) = the first such query -- or a part the
 * archive does not hold, a NULL that is needed (*bad_query = -1). */
typedef struct agc_ranges_t agc_ranges_t;
typedef struct {
    uint64_t n_q, n_win, n_parts, src_bytes;
    const uint8_t *src;
    const uint64_t *q_seg; /* n_q + 1 */
    const uint64_t *q_len; /* n_q */
    const uint32_t *group_id, *in_group_id, *rc, *length, *kind, *seg_part, *seg_index, *win_from, *win_len; /* n_win each */
    const uint64_t *part_off;                                                                                  /* n_parts */
    const uint32_t *part_bytes, *part_coding, *part_content, *part_group, *part_no;                            /* n_parts each */
} agc_ranges_view;
agc_ranges_t *agc_get_range_parts(const agc_t *agc, uint64_t n_q, const char *const *samples, const char *const *names, const int64_t *from, const int64_t *to,
                                  const uint32_t *have_groups, uint64_t n_have, int64_t *bad_query);
/* fills *out; 0 for success */
int agc_ranges_fields(const agc_ranges_t *ranges, agc_ranges_view *out);
/* frees the ranges object (NULL: nothing to do); returns 0 */
int agc_ranges_destroy(agc_ranges_t *ranges);

#ifdef __cplusplus
}
#endif
#endif
