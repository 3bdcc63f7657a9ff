// read_api.hip -- the read path of include/agc_hip.h on the context's first stream: agc_hip_zstd_decode_batch (frames -> bytes),
// agc_hip_lz_decode_batch (deltas -> symbols), agc_hip_sample_fasta (a sample's plan -> its FASTA text), agc_hip_parts_unpack
// (archive parts -> packs cut into sequences, references as symbols), agc_hip_sample_fasta_parts (a sample's archive parts -> its
// FASTA text), agc_hip_lz_decode_window_batch (deltas -> a window of each one's symbols) and agc_hip_ranges_parts (archive parts -> a
// batch of contig ranges), each with its _dev twin, and agc_hip_bgzf (bytes -> a BGZF stream) with agc_hip_sample_fasta_parts_bgzf (a
// sample's archive parts -> its FASTA text as a BGZF stream) and agc_hip_bgzf_inflate (a BGZF stream -> its bytes; the walk of the
// stream and the decoder are inflate.h, the kernel inflate_kernels.hip).  All are built from the stages below.  The host arithmetic is not here:
// layout, jobs and first complaint of a sample are fasta_plan.h's, of a range batch range_plan.h's (both run on the CPU in tests/);
// this file checks arguments, uploads, launches and copies back.  The two calls from archive parts share PartsCall, the two LZ
// decode calls scan_delta_batch.  Included by api.hip behind the create path (uses its context and helpers; the kernels are
// lz_decode_kernels.hip, fasta_out_kernels.hip, zstd_decode_kernels.hip, parts_unpack_kernels.hip, range_kernels.hip, bgzf_kernels.hip).
#include <map>

#include "fasta_plan.h"
#include "range_plan.h"

namespace {

// ---- checks: the message begins with the call's name ----------------------------------------------------------------------------
int refuse(agc_hip_ctx *c, const std::string &what, int code = AGC_HIP_EINVAL)
{
    c->err = what;
    return code;
}

// item i of a batch (a "delta", a "frame") lies at [off[i], off[i + 1])
int offsets_ascend(agc_hip_ctx *c, const char *call, const char *item, const uint64_t *off, uint32_t i)
{
    return off[i + 1] >= off[i] ? AGC_HIP_OK : refuse(c, std::string(call) + ": " + item + " " + std::to_string(i) + " ends in front of its start");
}

// the caller's buffer (the "output" buffer, the "text" buffer) has room for what the call is about to write
int capacity_holds(agc_hip_ctx *c, const char *call, const char *buffer, uint64_t cap, uint64_t need)
{
    return need <= cap ? AGC_HIP_OK : refuse(c, std::string(call) + ": the " + buffer + " buffer holds " + std::to_string(cap) + " bytes, " + std::to_string(need) + " are needed", AGC_HIP_ECAP);
}

// the group has a registered reference; the symbols of it, -1: it has none
bool registered(const agc_hip_ctx *c, uint32_t gid) { return gid < c->refs.size() && c->refs[gid].valid; }
int64_t registered_size(const agc_hip_ctx *c, uint32_t gid) { return registered(c, gid) ? (int64_t)c->refs[gid].ref_size : (int64_t)-1; }

// A launch that gives every 16-byte chunk of what it writes a lane, 256 to a block.  add(): `bytes` bytes at address p join it (a: that
// address's alignment) -> the piece's first chunk.  A launch of one piece is {a, n_chunks, blocks} after one add().
struct ChunkLaunch {
    uint32_t a = 0; // of the piece added LAST: a launch of several pieces copies it after every add()
    uint64_t n_chunks = 0, blocks = 0;
    uint64_t add(const void *p, uint64_t bytes)
    {
        const uint64_t first = n_chunks;
        a = (uint32_t)((uintptr_t)p & (fo::CHUNK - 1));
        n_chunks += fo::chunk_count(a, bytes);
        blocks = (n_chunks + 255) / 256;
        return first;
    }
    // `what` ("sample_fasta: a text of 5 bytes is") more than one launch `does`
    int fits(agc_hip_ctx *c, const std::string &what, const char *does) const { return blocks <= 0x7FFFFFFFull ? AGC_HIP_OK : refuse(c, what + " more than one launch " + does); }
};

// ---- stages -------------------------------------------------------------------------------------------------------------------------
// where a call writes: the caller's device buffer, or -- d_out == nullptr -- the context's, grown to hold `bytes`
int output_buffer(agc_hip_ctx *c, uint8_t *&d_out, DevBuf &own, uint64_t bytes)
{
    if (!d_out) {
        CHK(ensure(c, own, bytes + 64));
        d_out = own.as<uint8_t>();
    }
    return AGC_HIP_OK;
}

// the end of a call: what was written goes to the host when the caller asked for it there, and the stream is waited for
int hand_back(agc_hip_ctx *c, uint8_t *h_out, const uint8_t *d_out, uint64_t bytes)
{
    if (h_out && bytes)
        HIPCHK(c, hipMemcpyAsync(h_out, d_out, bytes, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return AGC_HIP_OK;
}

// The scan stage: the jobs go up, lz_decode_scan_kernel walks every delta (they lie in d_enc already, a wave per delta) and the
// host waits for each one's length and status.
int decode_scan(agc_hip_ctx *c, const std::vector<DecodeJob> &jobs, const uint8_t *d_enc, std::vector<DecodeResult> &res)
{
    const uint32_t n = (uint32_t)jobs.size();
    CHK(ensure(c, c->rd.d_dec_jobs, (size_t)n * sizeof(DecodeJob)));
    CHK(ensure(c, c->rd.d_dec_res, (size_t)n * sizeof(DecodeResult)));
    CHK(upload(c, c->rd.d_dec_jobs.p, jobs.data(), (size_t)n * sizeof(DecodeJob), c->stream));
    {
        KTimer t(c, AGC_HIP_K_DECODE_SCAN);
        hipLaunchKernelGGL(lz_decode_scan_kernel, dim3((n + 3) / 4), dim3(4 * WAVE), 0, c->stream, (const RefDesc *)c->d_refs.p, (const DecodeJob *)c->rd.d_dec_jobs.p, n,
                           d_enc, (DecodeResult *)c->rd.d_dec_res.p);
    }
    HIPCHK(c, hipGetLastError());
    res.resize(n);
    HIPCHK(c, hipMemcpyAsync(res.data(), c->rd.d_dec_res.p, (size_t)n * sizeof(DecodeResult), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return AGC_HIP_OK;
}

// The write stage: lz_decode_write_kernel decodes the n jobs in d_dec_jobs -- scanned, and now saying where each delta's symbols go
// -- out of d_enc into d_out.
int decode_write(agc_hip_ctx *c, uint32_t n, const uint8_t *d_enc, uint8_t *d_out)
{
    {
        KTimer t(c, AGC_HIP_K_DECODE_WRITE);
        hipLaunchKernelGGL(lz_decode_write_kernel, dim3((n + 3) / 4), dim3(4 * WAVE), 0, c->stream, (const RefDesc *)c->d_refs.p, (const DecodeJob *)c->rd.d_dec_jobs.p, n,
                           d_enc, d_out);
    }
    HIPCHK(c, hipGetLastError());
    return AGC_HIP_OK;
}

// The scan stage with its verdict on deltas whose lengths a plan declares (job i: out_len, and the segment or window -- `noun` --
// item[i] it belongs to): every one well formed and of that length, or the first that is not is named.  No job: no launch.
int scan_declared_lengths(agc_hip_ctx *c, const char *call, const char *noun, const std::vector<DecodeJob> &jobs, const std::vector<uint32_t> &item, const uint8_t *d_bytes)
{
    if (jobs.empty())
        return AGC_HIP_OK;
    std::vector<DecodeResult> res;
    CHK(decode_scan(c, jobs, d_bytes, res));
    for (size_t i = 0; i < jobs.size(); ++i)
        if (res[i].status != lzd::OK || res[i].len != jobs[i].out_len)
            return refuse(c, std::string(call) + ": " + noun + " " + std::to_string(item[i]) +
                                 (res[i].status != lzd::OK ? " has a malformed delta" : " has a delta that decodes to " + std::to_string(res[i].len) + " symbols, its length says " + std::to_string(jobs[i].out_len)));
    return AGC_HIP_OK;
}

// how fasta_text_kernel is launched for a text of `text` bytes at d_text (nullptr: the context's buffer, which is aligned)
int text_launch(agc_hip_ctx *c, const uint8_t *d_text, uint64_t text, ChunkLaunch &T)
{
    T.add(d_text, text);
    return T.fits(c, "sample_fasta: a text of " + std::to_string(text) + " bytes is", "writes");
}

using SampleLayout = fp::SampleLayout<DecodeJob, CopyJob>;

// The sample stage: everything behind a sample's layout Y, its deltas and raw symbols in d_bytes already.  The deltas are checked by
// the scan stage, against the length the plan declares, before anything is written: the write stage and segment_copy_kernel then lay
// the segments out in the symbol buffer, fasta_text_kernel writes the text.
int write_sample(agc_hip_ctx *c, const SampleLayout &Y, const uint8_t *d_bytes, uint32_t n_ctg, const uint64_t *h_ctg_seg, const char *h_names,
                 const uint64_t *h_name_off, uint32_t line_length, uint8_t *h_text, uint8_t *d_text, const ChunkLaunch &T)
{
    CHK(upload_refs(c));
    const uint32_t n_dj = (uint32_t)Y.dj.size(), n_cj = (uint32_t)Y.cj.size();
    CHK(scan_declared_lengths(c, "sample_fasta", "segment", Y.dj, Y.dj_seg, d_bytes));
    // every segment has passed: from here on things are written
    CHK(ensure(c, c->rd.d_fa_sym, Y.sym_total + 64));
    uint8_t *d_sym = c->rd.d_fa_sym.as<uint8_t>();
    if (n_dj)
        CHK(decode_write(c, n_dj, d_bytes, d_sym));
    if (n_cj) {
        CHK(ensure(c, c->rd.d_fa_copy, (size_t)n_cj * sizeof(CopyJob)));
        CHK(upload(c, c->rd.d_fa_copy.p, Y.cj.data(), (size_t)n_cj * sizeof(CopyJob), c->stream));
        KTimer t(c, AGC_HIP_K_FASTA_OUT);
        hipLaunchKernelGGL(segment_copy_kernel, dim3((n_cj + 3) / 4), dim3(4 * WAVE), 0, c->stream, (const RefDesc *)c->d_refs.p, (const CopyJob *)c->rd.d_fa_copy.p, n_cj,
                           d_bytes, d_sym); // a wave per segment
    }
    HIPCHK(c, hipGetLastError());
    const fp::PlanBlock B = fp::pack_text_plan(Y, n_ctg, h_ctg_seg, h_names, h_name_off);
    CHK(ensure(c, c->rd.d_fa_plan, B.bytes.size() + 64));
    CHK(upload(c, c->rd.d_fa_plan.p, B.bytes.data(), B.bytes.size(), c->stream));
    CHK(output_buffer(c, d_text, c->rd.d_fa_text, Y.text));
    const uint8_t *pl = c->rd.d_fa_plan.as<uint8_t>();
    const TextPlan P = {(g_u64 *)(pl + B.ctg_text), (g_u64 *)(pl + B.ctg_seg), (g_u64 *)(pl + B.ctg_sym), (g_u64 *)(pl + B.name_off), (g_u8 *)(pl + B.names),
                        (g_u64 *)(pl + B.seg_start), (g_u64 *)(pl + B.seg_off), (g_u32 *)(pl + B.skip), (g_u8 *)d_sym, n_ctg, line_length};
    {
        KTimer t(c, AGC_HIP_K_FASTA_OUT);
        hipLaunchKernelGGL(fasta_text_kernel, dim3((uint32_t)T.blocks), dim3(256), 0, c->stream, P, d_text, T.a, Y.text, T.n_chunks);
    }
    HIPCHK(c, hipGetLastError());
    return hand_back(c, h_text, d_text, Y.text);
}

// The zstd stage: the frames lie in d_src already, their headers read by the host.  zstd_decode_kernel gives every job a wave, its
// slice of d_out and its slice of the literals workspace (ws_tot bytes in all); a job whose header the host refused only hands its
// status on.  The statuses stay in d_zd_status, one per job.
int zstd_decode_stage(agc_hip_ctx *c, const std::vector<ZDecJob> &jobs, uint64_t ws_tot, const uint8_t *d_src, uint8_t *d_out)
{
    const uint32_t n = (uint32_t)jobs.size();
    CHK(ensure(c, c->rd.d_zd_jobs, (size_t)n * sizeof(ZDecJob)));
    CHK(ensure(c, c->rd.d_zd_status, (size_t)n * sizeof(uint32_t)));
    CHK(ensure(c, c->rd.d_zd_ws, ws_tot + 64));
    CHK(upload(c, c->rd.d_zd_jobs.p, jobs.data(), (size_t)n * sizeof(ZDecJob), c->stream));
    {
        KTimer t(c, AGC_HIP_K_ZSTD_DECODE);
        hipLaunchKernelGGL(zstd_decode_kernel, dim3(n), dim3(WAVE), 0, c->stream, (const ZDecJob *)c->rd.d_zd_jobs.p, n, d_src, d_out, (uint8_t *)c->rd.d_zd_ws.p,
                           (uint32_t *)c->rd.d_zd_status.p); // a wave per frame
    }
    HIPCHK(c, hipGetLastError());
    return AGC_HIP_OK;
}

// one frame's job from its header: where it lies in the source, where its bytes and its literals workspace (min(content size,
// 128 KiB): what a block's literals can need) begin
ZDecJob zstd_job(const zs::dec::FrameHeader &h, uint64_t src_off, uint64_t len, uint64_t out_off, uint64_t &ws_tot)
{
    const uint32_t ws_len = (std::min(h.contentSize, zs::BLOCKSIZE_MAX) + 15u) & ~15u;
    const ZDecJob jb = {src_off, out_off, ws_tot, (uint32_t)len, h.contentSize, ws_len, h.status};
    ws_tot += ws_len;
    return jb;
}

// ---- the parts stage -------------------------------------------------------------------------------------------------------------
// what it leaves: every part's decoded bytes in d_pu_dec (jobs[i].dec_off, 16-byte aligned, the STORED parts in front), and what the
// device found out about them
struct PartsState {
    std::vector<PartJob> jobs;
    std::vector<PartInfo> info;    // status; a pack's count; a reference's nb and symbols
    std::vector<uint32_t> seq_end; // jobs[i].seq_row * seq_cap + q: where sequence q of pack i ends
    uint32_t seq_cap = 0;
    uint64_t dec_bytes = 0;

    uint32_t status(uint32_t i) const { return info[i].status; }
    // sequence q of pack i, as bytes [off, off + n) of d_pu_dec; false: q is at or above the pack's count or seq_cap, `why` says so
    bool locate(uint32_t i, uint32_t q, uint64_t &off, uint32_t &n, std::string &why) const
    {
        if (q >= info[i].count || q >= seq_cap) {
            why = "sequence " + std::to_string(q) + " of part " + std::to_string(i) + ", which has " + std::to_string(info[i].count) + " (at most " + std::to_string(seq_cap) +
                  " are indexed)";
            return false;
        }
        const uint32_t *row = seq_end.data() + (size_t)jobs[i].seq_row * seq_cap;
        const uint32_t begin = q ? row[q - 1] + 1 : 0;
        off = jobs[i].dec_off + begin;
        n = row[q] - begin;
        return true;
    }
};

// the parts as arguments: inside the source, of a known coding and content
int parts_check(agc_hip_ctx *c, const char *call, uint32_t n, const agc_hip_part *h_parts, uint64_t src_bytes)
{
    for (uint32_t i = 0; i < n; ++i) {
        const agc_hip_part &p = h_parts[i];
        const char *why = p.off > src_bytes || p.n_bytes > src_bytes - p.off ? "lies outside the source buffer"
                          : p.coding > AGC_HIP_PART_ZSTD                    ? "has an unknown coding"
                          : p.content > AGC_HIP_PART_REF_TUPLES             ? "has an unknown content"
                                                                            : nullptr;
        if (why)
            return refuse(c, std::string(call) + ": part " + std::to_string(i) + " " + why);
    }
    return AGC_HIP_OK;
}

// The parts stage (n >= 1 checked parts): the ZSTD parts through the zstd stage into d_pu_dec, the STORED ones uploaded beside them;
// pack_index_kernel cuts the packs (a wave each), tuples_size_kernel reads the references' shapes; infos and end offsets come back
// in one copy, which the host waits for.
int parts_decode_index(agc_hip_ctx *c, uint32_t n, const agc_hip_part *h_parts, const uint8_t *h_src, uint32_t seq_cap, PartsState &S)
{
    S.jobs.assign(n, PartJob());
    S.seq_cap = seq_cap;
    std::vector<uint32_t> ids(n); // the packs' part numbers from the front, the references' from the back
    uint32_t n_packs = 0, n_refs = 0, n_live = 0;
    uint64_t tot = 0, ws_tot = 0;
    std::vector<uint8_t> stored, frames;
    std::vector<ZDecJob> zj;
    auto align = [](uint64_t x) { return (x + 15) & ~(uint64_t)15; };
    for (uint32_t i = 0; i < n; ++i) {
        const agc_hip_part &p = h_parts[i];
        PartJob &j = S.jobs[i];
        j.content = p.content;
        j.zd_slot = ~0u;
        if (p.content == AGC_HIP_PART_PACK) {
            j.seq_row = n_packs;
            ids[n_packs++] = i;
        } else
            ids[n - ++n_refs] = i;
        if (p.coding == AGC_HIP_PART_STORED) {
            j.dec_off = tot;
            j.dec_len = p.n_bytes;
            tot += align(p.n_bytes);
            stored.resize(tot);
            if (p.n_bytes)
                std::memcpy(stored.data() + j.dec_off, h_src + p.off, p.n_bytes);
        }
    }
    for (uint32_t i = 0; i < n; ++i) {
        const agc_hip_part &p = h_parts[i];
        if (p.coding != AGC_HIP_PART_ZSTD)
            continue;
        PartJob &j = S.jobs[i];
        const zs::dec::FrameHeader h = zs::dec::parseFrameHeader(h_src + p.off, p.n_bytes);
        j.status = h.status;
        j.dec_off = tot;
        j.dec_len = h.status == zs::dec::OK ? h.contentSize : 0;
        j.zd_slot = (uint32_t)zj.size();
        zj.push_back(zstd_job(h, frames.size(), p.n_bytes, tot, ws_tot));
        frames.insert(frames.end(), h_src + p.off, h_src + p.off + p.n_bytes);
        tot += align(j.dec_len);
        n_live += h.status == zs::dec::OK;
    }
    if (!n_live) // (every header refused, or no ZSTD part: the zstd stage does not run and leaves no status to read)
        for (PartJob &j : S.jobs)
            j.zd_slot = ~0u;
    S.dec_bytes = tot;
    CHK(ensure(c, c->rd.d_pu_dec, tot + 64));
    uint8_t *d_dec = c->rd.d_pu_dec.as<uint8_t>();
    if (!stored.empty())
        CHK(upload(c, d_dec, stored.data(), stored.size(), c->stream));
    if (n_live) {
        CHK(ensure(c, c->rd.d_zd_src, frames.size() + 64));
        CHK(upload(c, c->rd.d_zd_src.p, frames.data(), frames.size(), c->stream));
        CHK(zstd_decode_stage(c, zj, ws_tot, c->rd.d_zd_src.as<uint8_t>(), d_dec));
    }
    // descriptors and part numbers in one block up, infos and end offsets in one block down
    const size_t jobs_bytes = (size_t)n * sizeof(PartJob), info_bytes = (size_t)n * sizeof(PartInfo), ends = (size_t)n_packs * seq_cap;
    std::vector<uint8_t> up(jobs_bytes + (size_t)n * 4), down(info_bytes + ends * 4);
    std::memcpy(up.data(), S.jobs.data(), jobs_bytes);
    std::memcpy(up.data() + jobs_bytes, ids.data(), (size_t)n * 4);
    CHK(ensure(c, c->rd.d_pu_jobs, up.size()));
    CHK(ensure(c, c->rd.d_pu_res, down.size() + 64));
    CHK(upload(c, c->rd.d_pu_jobs.p, up.data(), up.size(), c->stream));
    const PartJob *d_jobs = c->rd.d_pu_jobs.as<PartJob>();
    const uint32_t *d_ids = (const uint32_t *)(c->rd.d_pu_jobs.as<uint8_t>() + jobs_bytes);
    PartInfo *d_info = c->rd.d_pu_res.as<PartInfo>();
    uint32_t *d_ends = (uint32_t *)(c->rd.d_pu_res.as<uint8_t>() + info_bytes);
    const uint32_t *d_zst = (const uint32_t *)c->rd.d_zd_status.p; // (read only through a zd_slot the zstd stage filled)
    if (n_packs) {
        KTimer t(c, AGC_HIP_K_PARTS_UNPACK);
        hipLaunchKernelGGL(pack_index_kernel, dim3((n_packs + 3) / 4), dim3(4 * WAVE), 0, c->stream, d_jobs, d_ids, n_packs, (const uint8_t *)d_dec, d_zst, seq_cap, d_ends,
                           d_info); // a wave per pack
    }
    if (n_refs) {
        KTimer t(c, AGC_HIP_K_PARTS_UNPACK);
        hipLaunchKernelGGL(tuples_size_kernel, dim3((n_refs + 255) / 256), dim3(256), 0, c->stream, d_jobs, d_ids + n_packs, n_refs, (const uint8_t *)d_dec, d_zst, d_info);
    }
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipMemcpyAsync(down.data(), c->rd.d_pu_res.p, down.size(), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    S.info.resize(n);
    std::memcpy(S.info.data(), down.data(), info_bytes);
    S.seq_end.resize(ends);
    if (ends)
        std::memcpy(S.seq_end.data(), down.data() + info_bytes, ends * 4);
    return AGC_HIP_OK;
}

// The unpack-write stage: tuples_unpack_kernel fills out[out_off, out_off + n) of every job -- symbols out of a tuple stream, or
// bytes as they are -- from d_pu_dec; the jobs (each with n >= 1) get their share of the launch's chunks here.
int unpack_write(agc_hip_ctx *c, std::vector<UnpackJob> &jobs, uint8_t *d_out)
{
    if (jobs.empty())
        return AGC_HIP_OK;
    ChunkLaunch L;
    for (UnpackJob &j : jobs) {
        j.first_chunk = L.add(d_out + j.out_off, j.n);
        j.a = L.a;
    }
    CHK(L.fits(c, "parts_unpack: " + std::to_string(L.n_chunks) + " chunks of 16 bytes are", "writes"));
    CHK(ensure(c, c->rd.d_pu_wjobs, jobs.size() * sizeof(UnpackJob)));
    CHK(upload(c, c->rd.d_pu_wjobs.p, jobs.data(), jobs.size() * sizeof(UnpackJob), c->stream));
    {
        KTimer t(c, AGC_HIP_K_PARTS_UNPACK);
        hipLaunchKernelGGL(tuples_unpack_kernel, dim3((uint32_t)L.blocks), dim3(256), 0, c->stream, (const UnpackJob *)c->rd.d_pu_wjobs.p, (uint32_t)jobs.size(), L.n_chunks,
                           (const uint8_t *)c->rd.d_pu_dec.p, d_out);
    }
    HIPCHK(c, hipGetLastError());
    return AGC_HIP_OK;
}

// The window-write stage: lz_decode_window_kernel writes the window of every delta job (scanned, the windows inside the lengths the
// scan reported) out of d_enc, segment_window_kernel the windows of the RAW (out of d_enc) and REF jobs, each straight to its place
// in d_out; letters_kernel then maps the `total` symbols at d_out to letters when asked to.
int window_write(agc_hip_ctx *c, const std::vector<WindowJob> &wj, const std::vector<WindowCopyJob> &cj, const uint8_t *d_enc, uint8_t *d_out, uint64_t total, bool letters)
{
    const uint32_t n_wj = (uint32_t)wj.size(), n_cj = (uint32_t)cj.size();
    ChunkLaunch L;
    L.add(d_out, total);
    CHK(L.fits(c, "ranges: " + std::to_string(total) + " symbols are", "maps to letters"));
    if (n_wj) {
        CHK(ensure(c, c->rd.d_rg_jobs, (size_t)n_wj * sizeof(WindowJob)));
        CHK(upload(c, c->rd.d_rg_jobs.p, wj.data(), (size_t)n_wj * sizeof(WindowJob), c->stream));
        KTimer t(c, AGC_HIP_K_RANGES);
        hipLaunchKernelGGL(lz_decode_window_kernel, dim3((n_wj + 3) / 4), dim3(4 * WAVE), 0, c->stream, (const RefDesc *)c->d_refs.p, (const WindowJob *)c->rd.d_rg_jobs.p, n_wj,
                           d_enc, d_out); // a wave per window
    }
    if (n_cj) {
        CHK(ensure(c, c->rd.d_rg_copy, (size_t)n_cj * sizeof(WindowCopyJob)));
        CHK(upload(c, c->rd.d_rg_copy.p, cj.data(), (size_t)n_cj * sizeof(WindowCopyJob), c->stream));
        KTimer t(c, AGC_HIP_K_RANGES);
        hipLaunchKernelGGL(segment_window_kernel, dim3((n_cj + 3) / 4), dim3(4 * WAVE), 0, c->stream, (const RefDesc *)c->d_refs.p, (const WindowCopyJob *)c->rd.d_rg_copy.p,
                           n_cj, d_enc, d_out);
    }
    if (letters && total) {
        KTimer t(c, AGC_HIP_K_RANGES);
        hipLaunchKernelGGL(letters_kernel, dim3((uint32_t)L.blocks), dim3(256), 0, c->stream, d_out, L.a, total, L.n_chunks);
    }
    HIPCHK(c, hipGetLastError());
    return AGC_HIP_OK;
}

// ---- the BGZF stage ----------------------------------------------------------------------------------------------------------------
// where a BGZF call leaves its stream: the caller's host or device buffer of `cap` bytes, its length, the members' offsets (optional)
struct GzOut {
    uint8_t *h_gz, *d_gz;
    uint64_t cap;
    uint64_t *h_len, *h_block_off;
};

// what can be said of a stream of `n` input bytes before anything is launched: the bound into *G.h_len; EINVAL for more blocks than
// a member count of 32 bits holds, ECAP when the bound does not fit
int bgzf_capacity(agc_hip_ctx *c, const char *call, uint64_t n, const GzOut &G)
{
    *G.h_len = bgzf::bound(n);
    if (bgzf::block_count(n) > 0xFFFFFFFFull)
        return refuse(c, std::string(call) + ": " + std::to_string(n) + " bytes are more than 2^32 - 1 blocks");
    return capacity_holds(c, call, "stream", G.cap, bgzf::bound(n));
}

// The BGZF stage: the n bytes at d_in (capacity checked) -> the stream.  bgzf_block_kernel leaves every block's member in its slot
// and its size beside it; the sizes come to the host -- the call's one copy down besides the stream itself --, which says where every
// member begins; bgzf_place_kernel moves them there and appends the EOF member.
int bgzf_stage(agc_hip_ctx *c, const char *call, const uint8_t *d_in, uint64_t n, const GzOut &G)
{
    const uint64_t n_blocks = bgzf::block_count(n);
    uint8_t *d_out = G.d_gz;
    CHK(output_buffer(c, d_out, c->rd.d_bz_out, bgzf::bound(n)));
    CHK(ensure(c, c->rd.d_bz_slots, n_blocks * bgzf::SLOT + 64));
    CHK(ensure(c, c->rd.d_bz_sizes, n_blocks * sizeof(uint32_t) + 64));
    CHK(ensure(c, c->rd.d_bz_off, (n_blocks + 1) * sizeof(uint64_t)));
    std::vector<uint32_t> sizes(n_blocks);
    std::vector<uint64_t> off(n_blocks + 1);
    if (n_blocks) {
        {
            KTimer t(c, AGC_HIP_K_BGZF);
            hipLaunchKernelGGL(bgzf_block_kernel, dim3((uint32_t)std::min<uint64_t>(n_blocks, 0x7FFFFFFFull)), dim3(bgzf::THREADS), 0, c->stream, d_in, n, n_blocks,
                               c->rd.d_bz_slots.as<uint8_t>(), c->rd.d_bz_sizes.as<uint32_t>()); // a workgroup per block
        }
        HIPCHK(c, hipGetLastError());
        HIPCHK(c, hipMemcpyAsync(sizes.data(), c->rd.d_bz_sizes.p, n_blocks * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
    }
    uint64_t at = 0;
    for (uint64_t b = 0; b < n_blocks; ++b) {
        if (sizes[b] < bgzf::HEADER + bgzf::TRAILER || sizes[b] > bgzf::MEMBER_MAX) // (no address is made of a size no member can have)
            return refuse(c, std::string(call) + ": block " + std::to_string(b) + " came back with a member of " + std::to_string(sizes[b]) + " bytes", AGC_HIP_ENODEV);
        off[b] = at;
        at += sizes[b];
    }
    off[n_blocks] = at;
    const uint64_t total = at + bgzf::EOF_BYTES; // (<= the bound: every member is at most its block + 31 bytes)
    CHK(upload(c, c->rd.d_bz_off.p, off.data(), off.size() * sizeof(uint64_t), c->stream));
    {
        KTimer t(c, AGC_HIP_K_BGZF);
        hipLaunchKernelGGL(bgzf_place_kernel, dim3((uint32_t)std::min<uint64_t>(n_blocks + 1, 0x7FFFFFFFull)), dim3(bgzf::THREADS), 0, c->stream,
                           (const uint8_t *)c->rd.d_bz_slots.p, (const uint32_t *)c->rd.d_bz_sizes.p, (const uint64_t *)c->rd.d_bz_off.p, n_blocks, d_out);
    }
    HIPCHK(c, hipGetLastError());
    *G.h_len = total;
    if (G.h_block_off)
        std::memcpy(G.h_block_off, off.data(), off.size() * sizeof(uint64_t));
    return hand_back(c, G.h_gz, d_out, total);
}

// The inflate stage: the stream lies in d_src already, walked by the host.  bgzf_inflate_kernel gives every member a wave and its
// slice of d_out; the statuses stay in d_inf_status, one per member.
int inflate_stage(agc_hip_ctx *c, const std::vector<inflate::Job> &jobs, const uint8_t *d_src, uint8_t *d_out)
{
    const uint32_t n = (uint32_t)jobs.size();
    CHK(ensure(c, c->rd.d_inf_jobs, (size_t)n * sizeof(inflate::Job)));
    CHK(ensure(c, c->rd.d_inf_status, (size_t)n * sizeof(uint32_t)));
    CHK(upload(c, c->rd.d_inf_jobs.p, jobs.data(), (size_t)n * sizeof(inflate::Job), c->stream));
    {
        KTimer t(c, AGC_HIP_K_INFLATE);
        hipLaunchKernelGGL(bgzf_inflate_kernel, dim3((n + INF_WAVES - 1) / INF_WAVES), dim3(INF_WAVES * WAVE), 0, c->stream, (const inflate::Job *)c->rd.d_inf_jobs.p, n, d_src,
                           d_out, (uint32_t *)c->rd.d_inf_status.p); // a wave per member
    }
    HIPCHK(c, hipGetLastError());
    return AGC_HIP_OK;
}

const char *inflate_refusal(uint32_t status) { return status == inflate::UNSUPPORTED ? "unsupported (status 1)" : "malformed (status 2)"; }

const char *delta_refusal(uint32_t status)
{
    static const char *why[] = {"", "a truncated or malformed token", "'!' at or past the end of the reference", "a match outside the reference",
                                "more than 2^32 - 1 decoded symbols"};
    return why[status <= lzd::TOO_LONG ? status : 1];
}

const char *part_refusal(uint32_t status)
{
    return status == pu::ZSTD_UNSUPPORTED ? "an unsupported zstd frame (status 1)" : status == pu::ZSTD_MALFORMED ? "a malformed zstd frame (status 2)" : "a malformed tuple stream (status 3)";
}

// ---- a call that reads from archive parts -------------------------------------------------------------------------------------------
// Steps 2 to 5 of agc_hip_sample_fasta_parts and agc_hip_ranges_parts (include/agc_hip.h), whose order is the contract: a group
// registers once, so no reference is registered until nothing can be refused any more.  A call makes one PartsCall and calls, in this
// order, check() -> unpack() -> its own layout, which may still refuse (locate() and ref_size() serve it) -> register_refs().
// Item: agc_hip_seg_part or agc_hip_seg_win (kind, gid, part, index, length, rc in front); noun: what a message calls one.
template <class Item> struct PartsCall {
    agc_hip_ctx *c;
    const char *call, *noun;
    uint32_t n_parts;
    const agc_hip_part *h_parts;
    const uint8_t *h_src;
    uint64_t src_bytes;
    uint32_t seq_cap, min_match_len;
    uint64_t n_items;
    const Item *h_items;
    PartsState S;
    std::map<uint32_t, uint32_t> new_ref; // group -> the part that is its NEW reference
    int refuse(const std::string &what, int code = AGC_HIP_EINVAL) { return ::refuse(c, std::string(call) + ": " + what, code); }

    // 2. Before any launch.  The parts as arguments; every REF_* part a new reference: of a group that is not registered and that no
    // other part names, with a min_match_len agc_hip_ref_register takes.  Every item; then extra(item) -> nullptr, or what else is wrong.
    template <class Extra> int check(Extra extra)
    {
        CHK(parts_check(c, call, n_parts, h_parts, src_bytes));
        for (uint32_t i = 0; i < n_parts; ++i)
            if (h_parts[i].content != AGC_HIP_PART_PACK) {
                const uint32_t g = h_parts[i].gid;
                if (registered(c, g) || !new_ref.emplace(g, i).second)
                    return refuse("part " + std::to_string(i) + " is a reference of group " + std::to_string(g) + ", which " +
                                  (registered(c, g) ? "is registered already" : "another part is a reference of as well"));
            }
        if (!new_ref.empty() && (min_match_len < HASHING_STEP + 4 || min_match_len > 32))
            return refuse("a min_match_len of " + std::to_string(min_match_len) + " registers no reference");
        for (uint64_t i = 0; i < n_items; ++i) {
            const Item &g = h_items[i];
            const char *why;
            int code = AGC_HIP_EINVAL;
            if (g.kind > AGC_HIP_SEG_DELTA)
                why = "has an unknown kind";
            else if (g.kind != AGC_HIP_SEG_RAW && !registered(c, g.gid) && !new_ref.count(g.gid))
                why = "names a group that has no registered reference and none among the parts", code = AGC_HIP_ENOREF;
            else if (g.kind != AGC_HIP_SEG_REF && (g.part >= n_parts || h_parts[g.part].content != AGC_HIP_PART_PACK))
                why = "names a part that is not a pack of the batch";
            else
                why = extra(g);
            if (why)
                return refuse(std::string(noun) + " " + std::to_string(i) + " " + why, code);
        }
        return AGC_HIP_OK;
    }

    // 3. The parts, unpacked on the device, and (4) what it found of them.  Nothing is registered or written yet.
    int unpack()
    {
        HIPCHK(c, hipSetDevice(c->device));
        if (n_parts)
            CHK(parts_decode_index(c, n_parts, h_parts, h_src, seq_cap, S));
        for (uint32_t i = 0; i < n_parts; ++i)
            if (S.status(i) != pu::OK || (h_parts[i].content != AGC_HIP_PART_PACK && S.info[i].n > 0xFFFFFFFFull))
                return refuse("part " + std::to_string(i) + " is refused: " + (S.status(i) != pu::OK ? part_refusal(S.status(i)) : "a reference of 2^32 symbols or more"));
        return AGC_HIP_OK;
    }

    // (4, for the call's layout) the sequence of RAW / DELTA item i, as bytes of d_pu_dec; EINVAL: its index is out of reach
    int locate(uint64_t i, uint64_t &off, uint32_t &n)
    {
        std::string why;
        return S.locate(h_items[i].part, h_items[i].index, off, n, why) ? AGC_HIP_OK : refuse(std::string(noun) + " " + std::to_string(i) + " is " + why);
    }
    // the symbols of a group's reference, new (as unpack() found it) or registered; -1: it has none
    int64_t ref_size(uint32_t gid) const { return new_ref.count(gid) ? (int64_t)S.info[new_ref.at(gid)].n : registered_size(c, gid); }

    // 5. The new references' symbols back to back (16-byte aligned) in the context's buffer, registered in one batch from there.
    int register_refs()
    {
        if (new_ref.empty())
            return AGC_HIP_OK;
        std::vector<UnpackJob> wj;
        std::vector<uint32_t> gid, len;
        std::vector<uint64_t> off;
        uint64_t tot = 0;
        for (const auto &gr : new_ref) {
            const PartJob &j = S.jobs[gr.second];
            const PartInfo &f = S.info[gr.second];
            gid.push_back(gr.first), off.push_back(tot), len.push_back((uint32_t)f.n);
            if (f.n)
                wj.push_back({j.dec_off, tot, f.n, 0, f.count, 0});
            tot += (f.n + 15) & ~(uint64_t)15;
        }
        CHK(ensure(c, c->rd.d_pu_out, tot + 64));
        CHK(unpack_write(c, wj, c->rd.d_pu_out.as<uint8_t>()));
        return agc_hip_ref_register_batch_dev(c, (uint32_t)gid.size(), gid.data(), c->rd.d_pu_out.as<uint8_t>(), off.data(), len.data(), nullptr, min_match_len);
    }
};

// The prelude of the two LZ decode calls, n >= 1 deltas: every group registered and the offsets ascending, or nothing is launched;
// then the jobs (their outputs not laid out yet), the deltas into d_dec_enc, the scan stage -- and the first delta it rejects.
int scan_delta_batch(agc_hip_ctx *c, const char *call, uint32_t n, const uint32_t *h_gid, const uint8_t *h_enc, const uint64_t *h_enc_off, const uint8_t *h_rc,
                     std::vector<DecodeJob> &jobs, std::vector<DecodeResult> &res)
{
    for (uint32_t i = 0; i < n; ++i) {
        if (!registered(c, h_gid[i]))
            return refuse(c, std::string(call) + ": delta " + std::to_string(i) + ": group " + std::to_string(h_gid[i]) + " has no registered reference");
        CHK(offsets_ascend(c, call, "delta", h_enc_off, i));
    }
    HIPCHK(c, hipSetDevice(c->device));
    CHK(upload_refs(c));
    const uint64_t e0 = h_enc_off[0], enc_bytes = h_enc_off[n] - e0;
    jobs.resize(n);
    for (uint32_t i = 0; i < n; ++i)
        jobs[i] = {h_enc_off[i] - e0, h_enc_off[i + 1] - h_enc_off[i], 0, 0, h_gid[i], h_rc && h_rc[i] ? 1u : 0u, 0};
    CHK(ensure(c, c->rd.d_dec_enc, enc_bytes + 64));
    if (enc_bytes)
        CHK(upload(c, c->rd.d_dec_enc.p, h_enc + e0, enc_bytes, c->stream));
    CHK(decode_scan(c, jobs, c->rd.d_dec_enc.as<uint8_t>(), res));
    for (uint32_t i = 0; i < n; ++i)
        if (res[i].status != lzd::OK)
            return refuse(c, std::string(call) + ": delta " + std::to_string(i) + " is rejected: " + delta_refusal(res[i].status));
    return AGC_HIP_OK;
}

// the job records range_plan.h and fasta_plan.h fill member by member, and tests/ranges_host and tests/fastaout_host mirror
static_assert(sizeof(DecodeJob) == 40 && sizeof(WindowJob) == 40 && sizeof(WindowCopyJob) == 40 && sizeof(CopyJob) == 32, "a job record changed: its CPU mirrors must follow");

} // namespace

// ---- the calls: each checks its arguments for both of its entry points, which differ in the one of h_out / d_out they pass on -------
// The LZ decode: the scan stage gives every delta's length and status, the host lays the output out, the write stage fills it --
// launched only when every delta of the batch is well formed.
static int lz_decode_impl(agc_hip_ctx *c, uint32_t n, const uint32_t *h_gid, const uint8_t *h_enc, const uint64_t *h_enc_off, const uint8_t *h_rc,
                          uint8_t *h_out, uint8_t *d_out, uint64_t out_cap, uint64_t *h_out_off)
{
    if (!c || !h_out_off || (n && (!h_gid || !h_enc_off || (h_enc_off[n] > h_enc_off[0] && !h_enc))) || (out_cap && !h_out && !d_out))
        return AGC_HIP_EINVAL;
    h_out_off[0] = 0;
    if (!n)
        return AGC_HIP_OK;
    std::vector<DecodeJob> jobs;
    std::vector<DecodeResult> res;
    CHK(scan_delta_batch(c, "lz_decode", n, h_gid, h_enc, h_enc_off, h_rc, jobs, res));
    uint64_t tot = 0;
    for (uint32_t i = 0; i < n; ++i) {
        h_out_off[i] = tot;
        jobs[i].out_off = tot;
        jobs[i].out_len = res[i].len;
        tot += res[i].len;
    }
    h_out_off[n] = tot;
    CHK(capacity_holds(c, "lz_decode", "output", out_cap, tot));
    if (!tot)
        return AGC_HIP_OK;
    CHK(output_buffer(c, d_out, c->rd.d_dec_out, tot));
    CHK(upload(c, c->rd.d_dec_jobs.p, jobs.data(), (size_t)n * sizeof(DecodeJob), c->stream)); // (now with where each delta's symbols go)
    CHK(decode_write(c, n, c->rd.d_dec_enc.as<uint8_t>(), d_out));
    return hand_back(c, h_out, d_out, tot);
}

// The FASTA text of a sample.  The layout -- and with it the text's size -- follows from the plan alone (fasta_plan.h); then the
// deltas are checked by the scan stage, against the length the plan declares, before anything is written: the write stage and
// segment_copy_kernel lay the segments out in the symbol buffer, fasta_text_kernel writes the text.
static int sample_fasta_impl(agc_hip_ctx *c, uint32_t n_ctg, const uint64_t *h_ctg_seg, const agc_hip_seg_src *h_seg, const uint8_t *h_bytes, uint64_t n_bytes,
                             uint32_t k, uint32_t line_length, const char *h_names, const uint64_t *h_name_off, uint8_t *h_text, uint8_t *d_text,
                             uint64_t text_cap, uint64_t *h_text_len)
{
    if (!c || !h_text_len || (n_ctg && (!h_ctg_seg || !h_name_off || (h_ctg_seg[n_ctg] && !h_seg) || (n_bytes && !h_bytes))) || (text_cap && !h_text && !d_text))
        return AGC_HIP_EINVAL;
    *h_text_len = 0;
    if (!n_ctg)
        return AGC_HIP_OK;
    const auto Y = fp::lay_out_sample<DecodeJob, CopyJob>(n_ctg, h_ctg_seg, h_seg, n_bytes, k, line_length, h_name_off, [c](uint32_t gid) { return registered_size(c, gid); });
    *h_text_len = Y.text;
    if (Y.code != AGC_HIP_OK)
        return refuse(c, Y.why, Y.code);
    CHK(capacity_holds(c, "sample_fasta", "text", text_cap, Y.text));
    ChunkLaunch T;
    CHK(text_launch(c, d_text, Y.text, T));
    HIPCHK(c, hipSetDevice(c->device));
    CHK(ensure(c, c->rd.d_dec_enc, n_bytes + 64));
    if (n_bytes)
        CHK(upload(c, c->rd.d_dec_enc.p, h_bytes, n_bytes, c->stream));
    return write_sample(c, Y, c->rd.d_dec_enc.as<uint8_t>(), n_ctg, h_ctg_seg, h_names, h_name_off, line_length, h_text, d_text, T);
}

// The zstd decode.  The host reads every frame header: that sizes the output, and a frame whose header is refused never reaches the
// decoder.  The zstd stage then gives every other frame a wave, its slice of the output and its slice of the literals workspace.
static int zstd_decode_impl(agc_hip_ctx *c, uint32_t n, const uint8_t *h_src, const uint64_t *h_src_off, uint8_t *h_out, uint8_t *d_out, uint64_t out_cap,
                            uint64_t *h_out_off, uint32_t *h_status)
{
    if (!c || !h_out_off || (n && (!h_src_off || (h_src_off[n] > h_src_off[0] && !h_src))) || (out_cap && !h_out && !d_out))
        return AGC_HIP_EINVAL;
    h_out_off[0] = 0;
    if (!n)
        return AGC_HIP_OK;
    for (uint32_t i = 0; i < n; ++i)
        CHK(offsets_ascend(c, "zstd_decode", "frame", h_src_off, i));
    const uint64_t s0 = h_src_off[0], src_bytes = h_src_off[n] - s0;
    std::vector<ZDecJob> jobs(n);
    uint64_t tot = 0, ws_tot = 0;
    uint32_t n_live = 0;
    for (uint32_t i = 0; i < n; ++i) {
        const uint64_t len = h_src_off[i + 1] - h_src_off[i];
        const zs::dec::FrameHeader h = zs::dec::parseFrameHeader(h_src + h_src_off[i], len);
        jobs[i] = zstd_job(h, h_src_off[i] - s0, len, tot, ws_tot);
        h_out_off[i] = tot;
        tot += h.contentSize;
        n_live += h.status == zs::dec::OK;
        if (h_status)
            h_status[i] = h.status;
    }
    h_out_off[n] = tot;
    CHK(capacity_holds(c, "zstd_decode", "output", out_cap, tot));
    std::vector<uint32_t> status(n);
    if (n_live) {
        HIPCHK(c, hipSetDevice(c->device));
        CHK(ensure(c, c->rd.d_zd_src, src_bytes + 64));
        // (an output of 0 bytes: the context's buffer stands in for a d_out the caller did not have to give)
        CHK(output_buffer(c, d_out, c->rd.d_zd_out, tot));
        CHK(upload(c, c->rd.d_zd_src.p, h_src + s0, src_bytes, c->stream));
        CHK(zstd_decode_stage(c, jobs, ws_tot, c->rd.d_zd_src.as<uint8_t>(), d_out));
        HIPCHK(c, hipMemcpyAsync(status.data(), c->rd.d_zd_status.p, (size_t)n * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
        CHK(hand_back(c, h_out, d_out, tot));
    } else
        for (uint32_t i = 0; i < n; ++i)
            status[i] = jobs[i].status;
    for (uint32_t i = 0; i < n; ++i)
        if (h_status)
            h_status[i] = status[i];
    for (uint32_t i = 0; i < n; ++i)
        if (status[i] != zs::dec::OK)
            return refuse(c, "zstd_decode: frame " + std::to_string(i) + " is refused: " + (status[i] == zs::dec::UNSUPPORTED ? "unsupported (status 1)" : "malformed (status 2)"));
    return AGC_HIP_OK;
}

// The parts of an archive into their final bytes.  The parts stage leaves everything decoded in the context's buffer and the host
// knowing every size; only then is the caller's capacity looked at and, when it holds, the unpack-write stage fills the output:
// a pack's and a byte reference's bytes as they are, a tuple reference's symbols.
static int parts_unpack_impl(agc_hip_ctx *c, uint32_t n, const agc_hip_part *h_parts, const uint8_t *h_src, uint64_t src_bytes, uint32_t seq_cap, uint8_t *h_out,
                             uint8_t *d_out, uint64_t out_cap, uint64_t *h_out_off, uint32_t *h_count, uint32_t *h_seq_end, uint32_t *h_status)
{
    if (!c || !h_out_off || (n && (!h_parts || !h_count || !h_status || (seq_cap && !h_seq_end) || (src_bytes && !h_src))) || (out_cap && !h_out && !d_out))
        return AGC_HIP_EINVAL;
    h_out_off[0] = 0;
    if (!n)
        return AGC_HIP_OK;
    CHK(parts_check(c, "parts_unpack", n, h_parts, src_bytes));
    HIPCHK(c, hipSetDevice(c->device));
    PartsState S;
    CHK(parts_decode_index(c, n, h_parts, h_src, seq_cap, S));
    std::vector<UnpackJob> wj;
    uint64_t tot = 0;
    for (uint32_t i = 0; i < n; ++i) {
        const PartJob &j = S.jobs[i];
        const PartInfo &f = S.info[i];
        const bool pack = j.content == AGC_HIP_PART_PACK;
        h_status[i] = f.status;
        h_out_off[i] = tot;
        if (f.status != pu::OK)
            continue;
        const uint64_t bytes = pack ? j.dec_len : f.n;
        if (bytes)
            wj.push_back({j.dec_off, tot, bytes, 0, pack ? 0u : f.count, 0});
        tot += bytes;
        if (pack) {
            h_count[i] = f.count;
            const uint32_t stored = std::min(f.count, seq_cap);
            if (stored)
                std::memcpy(h_seq_end + (size_t)i * seq_cap, S.seq_end.data() + (size_t)j.seq_row * seq_cap, (size_t)stored * 4);
        }
    }
    h_out_off[n] = tot;
    CHK(capacity_holds(c, "parts_unpack", "output", out_cap, tot));
    if (tot) {
        CHK(output_buffer(c, d_out, c->rd.d_pu_out, tot));
        CHK(unpack_write(c, wj, d_out));
        CHK(hand_back(c, h_out, d_out, tot));
    }
    for (uint32_t i = 0; i < n; ++i)
        if (h_status[i] != pu::OK)
            return refuse(c, "parts_unpack: part " + std::to_string(i) + " is refused: " + part_refusal(h_status[i]));
    return AGC_HIP_OK;
}

// The FASTA text of a sample from its archive parts: the order of events is the contract (include/agc_hip.h).  Everything the host
// can refuse is refused before the references are registered -- a group registers once, so a call that fails before that leaves the
// context as it found it; behind the registration only the deltas themselves can still be refused.
static int sample_fasta_parts_impl(agc_hip_ctx *c, uint32_t n_parts, const agc_hip_part *h_parts, const uint8_t *h_src, uint64_t src_bytes, uint32_t seq_cap,
                                   uint32_t n_ctg, const uint64_t *h_ctg_seg, const agc_hip_seg_part *h_seg, uint32_t k, uint32_t min_match_len, uint32_t line_length,
                                   const char *h_names, const uint64_t *h_name_off, uint8_t *h_text, uint8_t *d_text, uint64_t text_cap, uint64_t *h_text_len,
                                   const GzOut *gz = nullptr)
{
    // gz (agc_hip_sample_fasta_parts_bgzf): the text stays in the context's buffer (h_text, d_text and text_cap are not looked at) and
    // goes through the BGZF stage from there; the capacity that is checked in step 1 is the stream's
    static const char *call = "sample_fasta_parts";
    if (!c || !h_text_len || (n_ctg && (!h_ctg_seg || !h_name_off || (h_ctg_seg[n_ctg] && !h_seg))) || (n_parts && (!h_parts || (src_bytes && !h_src))) ||
        (gz ? !gz->h_len || (gz->cap && !gz->h_gz && !gz->d_gz) : text_cap && !h_text && !d_text))
        return AGC_HIP_EINVAL;
    *h_text_len = 0;
    if (!n_ctg) {
        if (!gz)
            return AGC_HIP_OK;
        CHK(bgzf_capacity(c, call, 0, *gz));
        HIPCHK(c, hipSetDevice(c->device));
        return bgzf_stage(c, call, nullptr, 0, *gz);
    }
    // 1. the text's size
    uint64_t text = 0;
    if (!fp::plan_text_bytes(n_ctg, h_ctg_seg, k, line_length, h_name_off, [h_seg](uint64_t s) { return h_seg[s].length; }, text))
        return refuse(c, std::string(call) + ": the contigs' segment ranges or name offsets do not ascend from 0");
    *h_text_len = text;
    if (gz) {
        CHK(bgzf_capacity(c, call, text, *gz));
        h_text = d_text = nullptr;
    } else
        CHK(capacity_holds(c, call, "text", text_cap, text));
    ChunkLaunch T;
    CHK(text_launch(c, d_text, text, T));
    // 2. the plan against the parts and the context; 3. the parts, unpacked on the device
    const uint64_t n_seg = h_ctg_seg[n_ctg];
    PartsCall<agc_hip_seg_part> P = {c, call, "segment", n_parts, h_parts, h_src, src_bytes, seq_cap, min_match_len, n_seg, h_seg};
    CHK(P.check([](const agc_hip_seg_part &) -> const char * { return nullptr; })); // (a segment has no further check)
    CHK(P.unpack());
    // 4. the layout, with the sequences where the device found them and the new references' sizes
    std::vector<agc_hip_seg_src> seg(n_seg);
    for (uint64_t s = 0; s < n_seg; ++s) {
        const agc_hip_seg_part &g = h_seg[s];
        seg[s] = {g.kind, g.gid, 0, 0, g.length, g.rc, 0};
        if (g.kind != AGC_HIP_SEG_REF)
            CHK(P.locate(s, seg[s].off, seg[s].n_bytes));
    }
    const SampleLayout Y = fp::lay_out_sample<DecodeJob, CopyJob>(n_ctg, h_ctg_seg, seg.data(), P.S.dec_bytes, k, line_length, h_name_off, [&P](uint32_t gid) { return P.ref_size(gid); });
    if (Y.code != AGC_HIP_OK)
        return refuse(c, Y.why, Y.code);
    // 5. the new references, registered in one batch from the device buffer
    CHK(P.register_refs());
    // 6. agc_hip_sample_fasta's path, the deltas and raw symbols read where the parts stage left them
    CHK(write_sample(c, Y, c->rd.d_pu_dec.as<uint8_t>(), n_ctg, h_ctg_seg, h_names, h_name_off, line_length, h_text, d_text, T));
    // 7. (gz) the text, which write_sample left in the context's buffer, into the stream
    return gz ? bgzf_stage(c, call, c->rd.d_fa_text.as<uint8_t>(), Y.text, *gz) : AGC_HIP_OK;
}

// Bytes into a BGZF stream.  The bound follows from n alone, so the capacity is looked at before anything else; then the BGZF stage.
static int bgzf_impl(agc_hip_ctx *c, const uint8_t *h_in, const uint8_t *d_in, uint64_t n, const GzOut &G)
{
    if (!c || !G.h_len || (n && !h_in && !d_in) || (G.cap && !G.h_gz && !G.d_gz))
        return AGC_HIP_EINVAL;
    CHK(bgzf_capacity(c, "bgzf", n, G));
    HIPCHK(c, hipSetDevice(c->device));
    if (h_in && n) {
        CHK(ensure(c, c->rd.d_bz_in, n + 64));
        CHK(upload(c, c->rd.d_bz_in.p, h_in, n, c->stream));
        d_in = c->rd.d_bz_in.as<uint8_t>();
    }
    return bgzf_stage(c, "bgzf", d_in, n, G);
}

// A BGZF stream into its bytes.  The host walks the stream (inflate.h): that finds every member, sizes the output, and a stream the
// walk complains about never reaches the device.  The inflate stage then gives every member a wave and its slice of the output.
static int bgzf_inflate_impl(agc_hip_ctx *c, const uint8_t *h_in, uint64_t n, uint8_t *h_out, uint8_t *d_out, uint64_t out_cap, uint64_t *h_out_len, uint64_t *h_text_off,
                             uint32_t *h_status)
{
    if (!c || !h_out_len || (n && !h_in) || (out_cap && !h_out && !d_out))
        return AGC_HIP_EINVAL;
    inflate::Walk W;
    inflate::walk(h_in, n, nullptr, 0, W);
    if (W.n_members > 0xFFFFFFFFull)
        return refuse(c, "bgzf_inflate: " + std::to_string(W.n_members) + " members are more than 2^32 - 1");
    std::vector<inflate::Job> jobs(W.n_members);
    inflate::Walk W2;
    inflate::walk(h_in, n, jobs.data(), jobs.size(), W2);
    const uint32_t n_mem = (uint32_t)jobs.size();
    *h_out_len = W.text_bytes;
    for (uint32_t m = 0; m < n_mem; ++m) {
        if (h_text_off)
            h_text_off[m] = jobs[m].out_off;
        if (h_status)
            h_status[m] = inflate::OK;
    }
    if (h_text_off)
        h_text_off[n_mem] = W.text_bytes;
    if (W.why != inflate::W_OK) {
        if (h_status)
            h_status[n_mem] = inflate::status_of(W.why);
        return refuse(c, "bgzf_inflate: member " + std::to_string(n_mem) + " at byte " + std::to_string(W.at) + " is refused: " + inflate_refusal(inflate::status_of(W.why)));
    }
    CHK(capacity_holds(c, "bgzf_inflate", "output", out_cap, W.text_bytes));
    if (!n_mem)
        return AGC_HIP_OK;
    HIPCHK(c, hipSetDevice(c->device));
    CHK(ensure(c, c->rd.d_inf_in, n + 64));
    // (an output of 0 bytes: the context's buffer stands in for a d_out the caller did not have to give)
    CHK(output_buffer(c, d_out, c->rd.d_inf_out, W.text_bytes));
    CHK(upload(c, c->rd.d_inf_in.p, h_in, n, c->stream));
    CHK(inflate_stage(c, jobs, c->rd.d_inf_in.as<uint8_t>(), d_out));
    std::vector<uint32_t> status(n_mem);
    HIPCHK(c, hipMemcpyAsync(status.data(), c->rd.d_inf_status.p, (size_t)n_mem * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
    CHK(hand_back(c, h_out, d_out, W.text_bytes));
    for (uint32_t m = 0; m < n_mem; ++m)
        if (h_status)
            h_status[m] = status[m];
    for (uint32_t m = 0; m < n_mem; ++m)
        if (status[m] != inflate::OK)
            return refuse(c, "bgzf_inflate: member " + std::to_string(m) + " is refused: " + inflate_refusal(status[m]));
    return AGC_HIP_OK;
}

// The windowed LZ decode: the output's layout follows from the windows' sizes, so the capacity is looked at first; the scan stage
// then checks every delta and says how long it is, and only when every window lies inside its delta is anything written.
static int lz_decode_window_impl(agc_hip_ctx *c, uint32_t n, const uint32_t *h_gid, const uint8_t *h_enc, const uint64_t *h_enc_off, const uint8_t *h_rc,
                                 const uint32_t *h_win_from, const uint32_t *h_win_len, uint8_t *h_out, uint8_t *d_out, uint64_t out_cap, uint64_t *h_out_off)
{
    static const char *call = "lz_decode_window";
    if (!c || !h_out_off || (n && (!h_gid || !h_enc_off || !h_win_from || !h_win_len || (h_enc_off[n] > h_enc_off[0] && !h_enc))) || (out_cap && !h_out && !d_out))
        return AGC_HIP_EINVAL;
    h_out_off[0] = 0;
    if (!n)
        return AGC_HIP_OK;
    uint64_t tot = 0;
    for (uint32_t i = 0; i < n; ++i) {
        h_out_off[i] = tot;
        tot += h_win_len[i];
    }
    h_out_off[n] = tot;
    CHK(capacity_holds(c, call, "output", out_cap, tot));
    for (uint32_t i = 0; i < n; ++i)
        if (!h_win_len[i])
            return refuse(c, std::string(call) + ": delta " + std::to_string(i) + " has a window of no symbols");
    std::vector<DecodeJob> jobs;
    std::vector<DecodeResult> res;
    CHK(scan_delta_batch(c, call, n, h_gid, h_enc, h_enc_off, h_rc, jobs, res));
    std::vector<WindowJob> wj(n);
    for (uint32_t i = 0; i < n; ++i) {
        if (!rp::window_fits(h_win_from[i], h_win_len[i], res[i].len))
            return refuse(c, std::string(call) + ": delta " + std::to_string(i) + " decodes to " + std::to_string(res[i].len) + " symbols, its window [" +
                                 std::to_string(h_win_from[i]) + ", +" + std::to_string(h_win_len[i]) + ") reaches past them");
        wj[i] = {jobs[i].enc_off, jobs[i].enc_len, h_out_off[i], 0, 0, jobs[i].ref_slot, jobs[i].rc};
        rw::decode_window(h_win_from[i], h_win_len[i], res[i].len, jobs[i].rc, wj[i].w_lo, wj[i].w_hi);
    }
    CHK(output_buffer(c, d_out, c->rd.d_rg_out, tot));
    CHK(window_write(c, wj, {}, c->rd.d_dec_enc.as<uint8_t>(), d_out, tot, false));
    return hand_back(c, h_out, d_out, tot);
}

// A batch of contig ranges from their archive parts: agc_hip_sample_fasta_parts's order of events (include/agc_hip.h) with windows in
// the place of whole segments -- everything the host can refuse is refused before the references are registered; behind the
// registration only the deltas themselves can still be refused.
static int ranges_parts_impl(agc_hip_ctx *c, uint32_t n_parts, const agc_hip_part *h_parts, const uint8_t *h_src, uint64_t src_bytes, uint32_t seq_cap, uint32_t n_q,
                             const uint64_t *h_q_seg, const agc_hip_seg_win *h_win, uint32_t min_match_len, int letters, uint8_t *h_out, uint8_t *d_out, uint64_t out_cap,
                             uint64_t *h_out_off)
{
    static const char *call = "ranges_parts";
    if (!c || !h_out_off || (n_q && (!h_q_seg || (h_q_seg[n_q] && !h_win))) || (n_parts && (!h_parts || (src_bytes && !h_src))) || (out_cap && !h_out && !d_out))
        return AGC_HIP_EINVAL;
    h_out_off[0] = 0;
    if (!n_q)
        return AGC_HIP_OK;
    // 1. the output's layout
    std::vector<uint64_t> win_out; // where every window goes
    uint64_t tot = 0;
    if (!rp::lay_out_queries(n_q, h_q_seg, h_win, h_out_off, win_out, tot))
        return refuse(c, std::string(call) + ": the queries' window ranges do not ascend from 0");
    CHK(capacity_holds(c, call, "output", out_cap, tot));
    // 2. the plan against the parts and the context, every window against its segment
    const uint64_t n_win = h_q_seg[n_q];
    PartsCall<agc_hip_seg_win> P = {c, call, "window", n_parts, h_parts, h_src, src_bytes, seq_cap, min_match_len, n_win, h_win};
    CHK(P.check([](const agc_hip_seg_win &g) -> const char * {
        return rp::window_fits(g.win_from, g.win_len, g.length) ? nullptr : g.win_len ? "reaches past its segment's length" : "has no symbols";
    }));
    if (!n_win)
        return AGC_HIP_OK;
    // 3. the parts, unpacked on the device
    CHK(P.unpack());
    // 4. the windows' jobs, with the sequences where the device found them and the new references' sizes
    const auto Y = rp::lay_out_windows<DecodeJob, WindowJob, WindowCopyJob>(
        call, n_win, h_win, win_out.data(), [&P](uint32_t part, uint32_t index, uint64_t &off, uint32_t &n, std::string &why) { return P.S.locate(part, index, off, n, why); },
        [&P](uint32_t gid) { return P.ref_size(gid); });
    if (Y.code != AGC_HIP_OK)
        return refuse(c, Y.why, Y.code);
    // 5. the new references, registered in one batch from the device buffer
    CHK(P.register_refs());
    // 6. the deltas against their lengths, then every window to its place
    CHK(upload_refs(c));
    const uint8_t *d_bytes = c->rd.d_pu_dec.as<uint8_t>();
    CHK(scan_declared_lengths(c, call, "window", Y.dj, Y.dj_win, d_bytes));
    CHK(output_buffer(c, d_out, c->rd.d_rg_out, tot));
    CHK(window_write(c, Y.wj, Y.cj, d_bytes, d_out, tot, letters != 0));
    return hand_back(c, h_out, d_out, tot);
}

extern "C" {

uint64_t agc_hip_bgzf_bound(uint64_t n_bytes) { return bgzf::bound(n_bytes); }

int agc_hip_bgzf(agc_hip_ctx *c, const uint8_t *h_in, uint64_t n, uint8_t *h_out, uint64_t out_cap, uint64_t *h_out_len, uint64_t *h_block_off)
{
    return bgzf_impl(c, h_in, nullptr, n, {h_out, nullptr, out_cap, h_out_len, h_block_off});
}

int agc_hip_bgzf_dev(agc_hip_ctx *c, const uint8_t *d_in, uint64_t n, uint8_t *d_out, uint64_t out_cap, uint64_t *h_out_len, uint64_t *h_block_off)
{
    return bgzf_impl(c, nullptr, d_in, n, {nullptr, d_out, out_cap, h_out_len, h_block_off});
}

int agc_hip_bgzf_members(const uint8_t *h_in, uint64_t n, uint64_t *h_n_members, uint64_t *h_text_bytes)
{
    if (!h_n_members || !h_text_bytes || (n && !h_in))
        return AGC_HIP_EINVAL;
    inflate::Walk W;
    inflate::walk(h_in, n, nullptr, 0, W);
    *h_n_members = W.n_members;
    *h_text_bytes = W.text_bytes;
    return W.why == inflate::W_OK ? AGC_HIP_OK : AGC_HIP_EINVAL;
}

int agc_hip_bgzf_inflate(agc_hip_ctx *c, const uint8_t *h_in, uint64_t n, uint8_t *h_out, uint64_t out_cap, uint64_t *h_out_len, uint64_t *h_text_off, uint32_t *h_status)
{
    return bgzf_inflate_impl(c, h_in, n, h_out, nullptr, out_cap, h_out_len, h_text_off, h_status);
}

int agc_hip_bgzf_inflate_dev(agc_hip_ctx *c, const uint8_t *h_in, uint64_t n, uint8_t *d_out, uint64_t out_cap, uint64_t *h_out_len, uint64_t *h_text_off, uint32_t *h_status)
{
    return bgzf_inflate_impl(c, h_in, n, nullptr, d_out, out_cap, h_out_len, h_text_off, h_status);
}

int agc_hip_sample_fasta_parts_bgzf(agc_hip_ctx *c, uint32_t n_parts, const agc_hip_part *h_parts, const uint8_t *h_src, uint64_t src_bytes, uint32_t seq_cap, uint32_t n_ctg,
                                    const uint64_t *h_ctg_seg, const agc_hip_seg_part *h_seg, uint32_t k, uint32_t min_match_len, uint32_t line_length, const char *h_names,
                                    const uint64_t *h_name_off, uint8_t *h_gz, uint64_t gz_cap, uint64_t *h_gz_len, uint64_t *h_text_len, uint64_t *h_block_off)
{
    const GzOut G = {h_gz, nullptr, gz_cap, h_gz_len, h_block_off};
    return sample_fasta_parts_impl(c, n_parts, h_parts, h_src, src_bytes, seq_cap, n_ctg, h_ctg_seg, h_seg, k, min_match_len, line_length, h_names, h_name_off, nullptr, nullptr,
                                   0, h_text_len, &G);
}

int agc_hip_sample_fasta_parts_bgzf_dev(agc_hip_ctx *c, uint32_t n_parts, const agc_hip_part *h_parts, const uint8_t *h_src, uint64_t src_bytes, uint32_t seq_cap,
                                        uint32_t n_ctg, const uint64_t *h_ctg_seg, const agc_hip_seg_part *h_seg, uint32_t k, uint32_t min_match_len, uint32_t line_length,
                                        const char *h_names, const uint64_t *h_name_off, uint8_t *d_gz, uint64_t gz_cap, uint64_t *h_gz_len, uint64_t *h_text_len,
                                        uint64_t *h_block_off)
{
    const GzOut G = {nullptr, d_gz, gz_cap, h_gz_len, h_block_off};
    return sample_fasta_parts_impl(c, n_parts, h_parts, h_src, src_bytes, seq_cap, n_ctg, h_ctg_seg, h_seg, k, min_match_len, line_length, h_names, h_name_off, nullptr, nullptr,
                                   0, h_text_len, &G);
}

int agc_hip_lz_decode_window_batch(agc_hip_ctx *c, uint32_t n, const uint32_t *h_gid, const uint8_t *h_enc, const uint64_t *h_enc_off, const uint8_t *h_rc,
                                   const uint32_t *h_win_from, const uint32_t *h_win_len, uint8_t *h_out, uint64_t out_cap, uint64_t *h_out_off)
{
    return lz_decode_window_impl(c, n, h_gid, h_enc, h_enc_off, h_rc, h_win_from, h_win_len, h_out, nullptr, out_cap, h_out_off);
}

int agc_hip_lz_decode_window_batch_dev(agc_hip_ctx *c, uint32_t n, const uint32_t *h_gid, const uint8_t *h_enc, const uint64_t *h_enc_off, const uint8_t *h_rc,
                                       const uint32_t *h_win_from, const uint32_t *h_win_len, uint8_t *d_out, uint64_t out_cap, uint64_t *h_out_off)
{
    return lz_decode_window_impl(c, n, h_gid, h_enc, h_enc_off, h_rc, h_win_from, h_win_len, nullptr, d_out, out_cap, h_out_off);
}

int agc_hip_ranges_parts(agc_hip_ctx *c, uint32_t n_parts, const agc_hip_part *h_parts, const uint8_t *h_src, uint64_t src_bytes, uint32_t seq_cap, uint32_t n_q,
                         const uint64_t *h_q_seg, const agc_hip_seg_win *h_win, uint32_t min_match_len, int letters, uint8_t *h_out, uint64_t out_cap, uint64_t *h_out_off)
{
    return ranges_parts_impl(c, n_parts, h_parts, h_src, src_bytes, seq_cap, n_q, h_q_seg, h_win, min_match_len, letters, h_out, nullptr, out_cap, h_out_off);
}

int agc_hip_ranges_parts_dev(agc_hip_ctx *c, uint32_t n_parts, const agc_hip_part *h_parts, const uint8_t *h_src, uint64_t src_bytes, uint32_t seq_cap, uint32_t n_q,
                             const uint64_t *h_q_seg, const agc_hip_seg_win *h_win, uint32_t min_match_len, int letters, uint8_t *d_out, uint64_t out_cap,
                             uint64_t *h_out_off)
{
    return ranges_parts_impl(c, n_parts, h_parts, h_src, src_bytes, seq_cap, n_q, h_q_seg, h_win, min_match_len, letters, nullptr, d_out, out_cap, h_out_off);
}

int agc_hip_lz_decode_batch(agc_hip_ctx *c, uint32_t n, const uint32_t *h_gid, const uint8_t *h_enc, const uint64_t *h_enc_off, const uint8_t *h_rc,
                            uint8_t *h_out, uint64_t out_cap, uint64_t *h_out_off)
{
    return lz_decode_impl(c, n, h_gid, h_enc, h_enc_off, h_rc, h_out, nullptr, out_cap, h_out_off);
}

int agc_hip_lz_decode_batch_dev(agc_hip_ctx *c, uint32_t n, const uint32_t *h_gid, const uint8_t *h_enc, const uint64_t *h_enc_off, const uint8_t *h_rc,
                                uint8_t *d_out, uint64_t out_cap, uint64_t *h_out_off)
{
    return lz_decode_impl(c, n, h_gid, h_enc, h_enc_off, h_rc, nullptr, d_out, out_cap, h_out_off);
}

int agc_hip_sample_fasta(agc_hip_ctx *c, uint32_t n_ctg, const uint64_t *h_ctg_seg, const agc_hip_seg_src *h_seg, const uint8_t *h_bytes, uint64_t n_bytes, uint32_t k,
                         uint32_t line_length, const char *h_names, const uint64_t *h_name_off, uint8_t *h_text, uint64_t text_cap, uint64_t *h_text_len)
{
    return sample_fasta_impl(c, n_ctg, h_ctg_seg, h_seg, h_bytes, n_bytes, k, line_length, h_names, h_name_off, h_text, nullptr, text_cap, h_text_len);
}

int agc_hip_sample_fasta_dev(agc_hip_ctx *c, uint32_t n_ctg, const uint64_t *h_ctg_seg, const agc_hip_seg_src *h_seg, const uint8_t *h_bytes, uint64_t n_bytes, uint32_t k,
                             uint32_t line_length, const char *h_names, const uint64_t *h_name_off, uint8_t *d_text, uint64_t text_cap, uint64_t *h_text_len)
{
    return sample_fasta_impl(c, n_ctg, h_ctg_seg, h_seg, h_bytes, n_bytes, k, line_length, h_names, h_name_off, nullptr, d_text, text_cap, h_text_len);
}

int agc_hip_zstd_decode_batch(agc_hip_ctx *c, uint32_t n, const uint8_t *h_src, const uint64_t *h_src_off, uint8_t *h_out, uint64_t out_cap, uint64_t *h_out_off,
                              uint32_t *h_status)
{
    return zstd_decode_impl(c, n, h_src, h_src_off, h_out, nullptr, out_cap, h_out_off, h_status);
}

int agc_hip_zstd_decode_batch_dev(agc_hip_ctx *c, uint32_t n, const uint8_t *h_src, const uint64_t *h_src_off, uint8_t *d_out, uint64_t out_cap, uint64_t *h_out_off,
                                  uint32_t *h_status)
{
    return zstd_decode_impl(c, n, h_src, h_src_off, nullptr, d_out, out_cap, h_out_off, h_status);
}

int agc_hip_parts_unpack(agc_hip_ctx *c, uint32_t n, const agc_hip_part *h_parts, const uint8_t *h_src, uint64_t src_bytes, uint32_t seq_cap, uint8_t *h_out,
                         uint64_t out_cap, uint64_t *h_out_off, uint32_t *h_count, uint32_t *h_seq_end, uint32_t *h_status)
{
    return parts_unpack_impl(c, n, h_parts, h_src, src_bytes, seq_cap, h_out, nullptr, out_cap, h_out_off, h_count, h_seq_end, h_status);
}

int agc_hip_parts_unpack_dev(agc_hip_ctx *c, uint32_t n, const agc_hip_part *h_parts, const uint8_t *h_src, uint64_t src_bytes, uint32_t seq_cap, uint8_t *d_out,
                             uint64_t out_cap, uint64_t *h_out_off, uint32_t *h_count, uint32_t *h_seq_end, uint32_t *h_status)
{
    return parts_unpack_impl(c, n, h_parts, h_src, src_bytes, seq_cap, nullptr, d_out, out_cap, h_out_off, h_count, h_seq_end, h_status);
}

int agc_hip_sample_fasta_parts(agc_hip_ctx *c, uint32_t n_parts, const agc_hip_part *h_parts, const uint8_t *h_src, uint64_t src_bytes, uint32_t seq_cap, uint32_t n_ctg,
                               const uint64_t *h_ctg_seg, const agc_hip_seg_part *h_seg, uint32_t k, uint32_t min_match_len, uint32_t line_length, const char *h_names,
                               const uint64_t *h_name_off, uint8_t *h_text, uint64_t text_cap, uint64_t *h_text_len)
{
    return sample_fasta_parts_impl(c, n_parts, h_parts, h_src, src_bytes, seq_cap, n_ctg, h_ctg_seg, h_seg, k, min_match_len, line_length, h_names, h_name_off, h_text, nullptr,
                                   text_cap, h_text_len);
}

int agc_hip_sample_fasta_parts_dev(agc_hip_ctx *c, uint32_t n_parts, const agc_hip_part *h_parts, const uint8_t *h_src, uint64_t src_bytes, uint32_t seq_cap, uint32_t n_ctg,
                                   const uint64_t *h_ctg_seg, const agc_hip_seg_part *h_seg, uint32_t k, uint32_t min_match_len, uint32_t line_length, const char *h_names,
                                   const uint64_t *h_name_off, uint8_t *d_text, uint64_t text_cap, uint64_t *h_text_len)
{
    return sample_fasta_parts_impl(c, n_parts, h_parts, h_src, src_bytes, seq_cap, n_ctg, h_ctg_seg, h_seg, k, min_match_len, line_length, h_names, h_name_off, nullptr, d_text,
                                   text_cap, h_text_len);
}

} // extern "C"
