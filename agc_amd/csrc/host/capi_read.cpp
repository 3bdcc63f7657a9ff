// capi_read.cpp -- C entry points of include/agc_read.h over agc::CAGCFile (reader.h).
// Mirrors src/lib-cxx/lib-cxx.cpp:123-330 of the reference (same names, same return conventions).
#include "reader.h"

#include <cstdlib>
#include <cstring>

#include "../../../include/agc_read.h"

struct agc_t {
    agc::CAGCFile f;
};

struct agc_plan_t {
    agc::SamplePlan p;
};

struct agc_parts_t {
    agc::SampleParts p;
};

struct agc_ranges_t {
    agc::RangeParts p;
};

static char **vec2list(const std::vector<std::string> &v)
{
    char **list = (char **)malloc(sizeof(char *) * (v.size() + 1));
    if (!list)
        return nullptr;
    for (size_t i = 0; i < v.size(); ++i) {
        list[i] = (char *)malloc(v[i].size() + 1);
        if (!list[i]) {
            for (size_t j = 0; j < i; ++j)
                free(list[j]);
            free(list);
            return nullptr;
        }
        memcpy(list[i], v[i].c_str(), v[i].size() + 1);
    }
    list[v.size()] = nullptr;
    return list;
}

extern "C" {

agc_t *agc_open(char *fn, int prefetching)
{
    if (!fn)
        return nullptr;
    agc_t *a = new agc_t;
    if (!a->f.Open(fn, prefetching != 0)) {
        delete a;
        return nullptr;
    }
    return a;
}

int agc_close(agc_t *agc)
{
    if (!agc)
        return -1;
    const bool r = agc->f.Close();
    delete agc;
    return r ? 0 : -1;
}

int agc_n_sample(const agc_t *agc) { return agc ? agc->f.NSample() : -1; }

int agc_get_ctg_seq(const agc_t *agc, const char *sample, const char *name, int start, int end, char *buf)
{
    if (!agc || !name || !buf)
        return -1;
    std::string s;
    if (agc->f.GetCtgSeq(sample ? sample : "", name, start, end, s) != 0)
        return -1;
    memcpy(buf, s.c_str(), s.size() + 1);
    return (int)s.size();
}

int agc_get_ctg_len(const agc_t *agc, const char *sample, const char *name)
{
    if (!agc || !name)
        return -1;
    return (int)agc->f.GetCtgLen(sample ? sample : "", name);
}

int agc_n_ctg(const agc_t *agc, const char *sample)
{
    if (!agc || !sample)
        return -1;
    return agc->f.NCtg(sample);
}

char *agc_reference_sample(const agc_t *agc)
{
    if (!agc)
        return nullptr;
    std::string s;
    if (agc->f.GetReferenceSample(s) < 0)
        return nullptr;
    char *c = (char *)malloc(s.size() + 1);
    if (c)
        memcpy(c, s.c_str(), s.size() + 1);
    return c;
}

char **agc_list_sample(const agc_t *agc, int *n_sample)
{
    if (!agc || !n_sample)
        return nullptr;
    std::vector<std::string> v;
    agc->f.ListSample(v);
    *n_sample = (int)v.size();
    return vec2list(v);
}

char **agc_list_ctg(const agc_t *agc, const char *sample, int *n_ctg)
{
    if (!agc || !sample || !n_ctg)
        return nullptr;
    std::vector<std::string> v;
    agc->f.ListCtg(sample, v);
    *n_ctg = (int)v.size();
    return vec2list(v);
}

int agc_list_destroy(char **list)
{
    if (!list)
        return 0;
    for (char **q = list; *q; ++q)
        free(*q);
    free(list);
    return 0;
}

int agc_string_destroy(char *sample)
{
    free(sample);
    return 0;
}

char *agc_get_sample_fasta(const agc_t *agc, const char *sample, int line_length, long long *len)
{
    if (!agc || !sample || !len)
        return nullptr;
    std::string s;
    if (!agc->f.GetSampleFasta(sample, s, line_length < 0 ? 0 : (uint32_t)line_length))
        return nullptr;
    char *c = (char *)malloc(s.size() + 1);
    if (!c)
        return nullptr;
    memcpy(c, s.c_str(), s.size() + 1);
    *len = (long long)s.size();
    return c;
}

int agc_get_params(const agc_t *agc, unsigned *k, unsigned *mml, unsigned *pack, unsigned *segment_size)
{
    if (!agc || !k || !mml || !pack || !segment_size)
        return -1;
    uint32_t a, b, c, d;
    if (!agc->f.GetParams(a, b, c, d))
        return -1;
    *k = a;
    *mml = b;
    *pack = c;
    *segment_size = d;
    return 0;
}

agc_plan_t *agc_get_sample_plan(const agc_t *agc, const char *sample)
{
    if (!agc || !sample)
        return nullptr;
    agc_plan_t *pl = new agc_plan_t;
    if (!agc->f.GetSamplePlan(sample, pl->p)) {
        delete pl;
        return nullptr;
    }
    return pl;
}

int agc_plan_fields(const agc_plan_t *plan, agc_plan_view *out)
{
    if (!plan || !out)
        return -1;
    const agc::SamplePlan &p = plan->p;
    out->n_ctg = p.ctg_seg.size() - 1;
    out->n_seg = p.kind.size();
    out->n_bytes = p.bytes.size();
    out->n_groups = p.groups.size();
    out->names = (const char *)p.names.data();
    out->name_off = p.name_off.data();
    out->ctg_seg = p.ctg_seg.data();
    out->group_id = p.group_id.data();
    out->in_group_id = p.in_group_id.data();
    out->rc = p.rc.data();
    out->length = p.length.data();
    out->kind = p.kind.data();
    out->seg_bytes = p.n_bytes.data();
    out->off = p.off.data();
    out->bytes = p.bytes.data();
    out->groups = p.groups.data();
    out->ref_off = p.ref_off.data();
    out->ref_bytes = p.ref_bytes.data();
    return 0;
}

int agc_plan_destroy(agc_plan_t *plan)
{
    delete plan;
    return 0;
}

agc_parts_t *agc_get_sample_parts(const agc_t *agc, const char *sample, const uint32_t *have_groups, uint64_t n_have)
{
    if (!agc || !sample || (n_have && !have_groups))
        return nullptr;
    agc_parts_t *pt = new agc_parts_t;
    if (!agc->f.GetSampleParts(sample, have_groups, (size_t)n_have, pt->p)) {
        delete pt;
        return nullptr;
    }
    return pt;
}

int agc_parts_fields(const agc_parts_t *parts, agc_parts_view *out)
{
    if (!parts || !out)
        return -1;
    const agc::SampleParts &p = parts->p;
    out->n_ctg = p.ctg_seg.size() - 1;
    out->n_seg = p.kind.size();
    out->n_parts = p.part_off.size();
    out->src_bytes = p.src_bytes;
    out->src = p.src;
    out->names = (const char *)p.names.data();
    out->name_off = p.name_off.data();
    out->ctg_seg = p.ctg_seg.data();
    out->group_id = p.group_id.data();
    out->in_group_id = p.in_group_id.data();
    out->rc = p.rc.data();
    out->length = p.length.data();
    out->kind = p.kind.data();
    out->seg_part = p.part.data();
    out->seg_index = p.index.data();
    out->part_off = p.part_off.data();
    out->part_bytes = p.part_bytes.data();
    out->part_coding = p.part_coding.data();
    out->part_content = p.part_content.data();
    out->part_group = p.part_group.data();
    out->part_no = p.part_no.data();
    return 0;
}

int agc_parts_destroy(agc_parts_t *parts)
{
    delete parts;
    return 0;
}

agc_ranges_t *agc_get_range_parts(const agc_t *agc, uint64_t n_q, const char *const *samples, const char *const *names, const int64_t *from, const int64_t *to,
                                  const uint32_t *have_groups, uint64_t n_have, int64_t *bad_query)
{
    if (bad_query)
        *bad_query = -1;
    if (!agc || (n_q && (!names || !from || !to)) || (n_have && !have_groups))
        return nullptr;
    std::vector<agc::RangeQuery> q((size_t)n_q);
    for (size_t i = 0; i < q.size(); ++i) {
        if (!names[i])
            return nullptr;
        q[i] = {samples && samples[i] ? samples[i] : "", names[i], from[i], to[i]};
    }
    agc_ranges_t *r = new agc_ranges_t;
    if (!agc->f.GetRangeParts(q, have_groups, (size_t)n_have, r->p, bad_query)) {
        delete r;
        return nullptr;
    }
    return r;
}

int agc_ranges_fields(const agc_ranges_t *ranges, agc_ranges_view *out)
{
    if (!ranges || !out)
        return -1;
    const agc::RangeParts &p = ranges->p;
    out->n_q = p.q_len.size();
    out->n_win = p.kind.size();
    out->n_parts = p.part_off.size();
    out->src_bytes = p.src_bytes;
    out->src = p.src;
    out->q_seg = p.q_seg.data();
    out->q_len = p.q_len.data();
    out->group_id = p.group_id.data();
    out->in_group_id = p.in_group_id.data();
    out->rc = p.rc.data();
    out->length = p.length.data();
    out->kind = p.kind.data();
    out->seg_part = p.part.data();
    out->seg_index = p.index.data();
    out->win_from = p.win_from.data();
    out->win_len = p.win_len.data();
    out->part_off = p.part_off.data();
    out->part_bytes = p.part_bytes.data();
    out->part_coding = p.part_coding.data();
    out->part_content = p.part_content.data();
    out->part_group = p.part_group.data();
    out->part_no = p.part_no.data();
    return 0;
}

int agc_ranges_destroy(agc_ranges_t *ranges)
{
    delete ranges;
    return 0;
}
}
