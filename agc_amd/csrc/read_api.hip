// read_api.hip -- the read path of include/agc_hip.h on the context's first stream: agc_hip_zstd_decode_batch (frames -> bytes),
// agc_hip_lz_decode_batch (deltas -> symbols) and agc_hip_sample_fasta (a sample's plan -> its FASTA text), each with its _dev twin.
// The three are built from the stages below; the sample's host arithmetic is fasta_plan.h.  Included by api.hip behind the create
// path (uses its context and helpers; the kernels are lz_decode_kernels.hip, fasta_out_kernels.hip, zstd_decode_kernels.hip).
#include "fasta_plan.h"

namespace {

// ---- checks: the message begins with the call's name ----------------------------------------------------------------------------
// item i of a batch (a "delta", a "frame") lies at [off[i], off[i + 1])
int offsets_ascend(agc_hip_ctx *c, const char *call, const char *item, const uint64_t *off, uint32_t i)
{
    if (off[i + 1] >= off[i])
        return AGC_HIP_OK;
    c->err = std::string(call) + ": " + item + " " + std::to_string(i) + " ends in front of its start";
    return AGC_HIP_EINVAL;
}

// the caller's buffer (the "output" buffer, the "text" buffer) has room for what the call is about to write
int capacity_holds(agc_hip_ctx *c, const char *call, const char *buffer, uint64_t cap, uint64_t need)
{
    if (need <= cap)
        return AGC_HIP_OK;
    c->err = std::string(call) + ": the " + buffer + " buffer holds " + std::to_string(cap) + " bytes, " + std::to_string(need) + " are needed";
    return AGC_HIP_ECAP;
}

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

// The scan stage: the jobs go up, lz_decode_scan_kernel walks every delta (they lie in d_dec_enc already, a wave per delta) and the
// host waits for each one's length and status.
int decode_scan(agc_hip_ctx *c, const std::vector<DecodeJob> &jobs, std::vector<DecodeResult> &res)
{
    const uint32_t n = (uint32_t)jobs.size();
    CHK(ensure(c, c->rd.d_dec_jobs, (size_t)n * sizeof(DecodeJob)));
    CHK(ensure(c, c->rd.d_dec_res, (size_t)n * sizeof(DecodeResult)));
    CHK(upload(c, c->rd.d_dec_jobs.p, jobs.data(), (size_t)n * sizeof(DecodeJob), c->stream));
    {
        KTimer t(c, AGC_HIP_K_DECODE_SCAN);
        hipLaunchKernelGGL(lz_decode_scan_kernel, dim3((n + 3) / 4), dim3(4 * WAVE), 0, c->stream, (const RefDesc *)c->d_refs.p, (const DecodeJob *)c->rd.d_dec_jobs.p, n,
                           (const uint8_t *)c->rd.d_dec_enc.p, (DecodeResult *)c->rd.d_dec_res.p);
    }
    HIPCHK(c, hipGetLastError());
    res.resize(n);
    HIPCHK(c, hipMemcpyAsync(res.data(), c->rd.d_dec_res.p, (size_t)n * sizeof(DecodeResult), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return AGC_HIP_OK;
}

// The write stage: lz_decode_write_kernel decodes the n jobs in d_dec_jobs -- scanned, and now saying where each delta's symbols go
// -- into d_out.
int decode_write(agc_hip_ctx *c, uint32_t n, uint8_t *d_out)
{
    {
        KTimer t(c, AGC_HIP_K_DECODE_WRITE);
        hipLaunchKernelGGL(lz_decode_write_kernel, dim3((n + 3) / 4), dim3(4 * WAVE), 0, c->stream, (const RefDesc *)c->d_refs.p, (const DecodeJob *)c->rd.d_dec_jobs.p, n,
                           (const uint8_t *)c->rd.d_dec_enc.p, d_out);
    }
    HIPCHK(c, hipGetLastError());
    return AGC_HIP_OK;
}

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
    for (uint32_t i = 0; i < n; ++i) {
        if (h_gid[i] >= c->refs.size() || !c->refs[h_gid[i]].valid) {
            c->err = "lz_decode: delta " + std::to_string(i) + ": group " + std::to_string(h_gid[i]) + " has no registered reference";
            return AGC_HIP_EINVAL;
        }
        CHK(offsets_ascend(c, "lz_decode", "delta", h_enc_off, i));
    }
    HIPCHK(c, hipSetDevice(c->device));
    CHK(upload_refs(c));
    const uint64_t e0 = h_enc_off[0], enc_bytes = h_enc_off[n] - e0;
    std::vector<DecodeJob> jobs(n);
    for (uint32_t i = 0; i < n; ++i)
        jobs[i] = {h_enc_off[i] - e0, h_enc_off[i + 1] - h_enc_off[i], 0, 0, h_gid[i], h_rc && h_rc[i] ? 1u : 0u, 0};
    CHK(ensure(c, c->rd.d_dec_enc, enc_bytes + 64));
    if (enc_bytes)
        CHK(upload(c, c->rd.d_dec_enc.p, h_enc + e0, enc_bytes, c->stream));
    std::vector<DecodeResult> res;
    CHK(decode_scan(c, jobs, res));
    for (uint32_t i = 0; i < n; ++i)
        if (res[i].status != lzd::OK) {
            static const char *why[] = {"", "a truncated or malformed token", "'!' at or past the end of the reference", "a match outside the reference",
                                        "more than 2^32 - 1 decoded symbols"};
            c->err = "lz_decode: delta " + std::to_string(i) + " is rejected: " + why[res[i].status <= lzd::TOO_LONG ? res[i].status : 1];
            return AGC_HIP_EINVAL;
        }
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
    CHK(decode_write(c, n, d_out));
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
    const auto Y = fp::lay_out_sample<DecodeJob, CopyJob>(n_ctg, h_ctg_seg, h_seg, n_bytes, k, line_length, h_name_off, [c](uint32_t gid) {
        return gid < c->refs.size() && c->refs[gid].valid ? (int64_t)c->refs[gid].ref_size : (int64_t)-1;
    });
    *h_text_len = Y.text;
    if (Y.code != AGC_HIP_OK) {
        c->err = Y.why;
        return Y.code;
    }
    CHK(capacity_holds(c, "sample_fasta", "text", text_cap, Y.text));
    const uint32_t a = d_text ? (uint32_t)((uintptr_t)d_text & (fo::CHUNK - 1)) : 0;
    const uint64_t n_chunks = fo::chunk_count(a, Y.text), text_blocks = (n_chunks + 255) / 256;
    if (text_blocks > 0x7FFFFFFFull) {
        c->err = "sample_fasta: a text of " + std::to_string(Y.text) + " bytes is more than one launch writes";
        return AGC_HIP_EINVAL;
    }
    HIPCHK(c, hipSetDevice(c->device));
    CHK(upload_refs(c));
    CHK(ensure(c, c->rd.d_dec_enc, n_bytes + 64));
    if (n_bytes)
        CHK(upload(c, c->rd.d_dec_enc.p, h_bytes, n_bytes, c->stream));
    const uint32_t n_dj = (uint32_t)Y.dj.size(), n_cj = (uint32_t)Y.cj.size();
    if (n_dj) {
        std::vector<DecodeResult> res;
        CHK(decode_scan(c, Y.dj, res));
        for (uint32_t i = 0; i < n_dj; ++i)
            if (res[i].status != lzd::OK || res[i].len != Y.dj[i].out_len) {
                c->err = "sample_fasta: segment " + std::to_string(Y.dj_seg[i]) +
                         (res[i].status != lzd::OK ? " has a malformed delta" : " decodes to " + std::to_string(res[i].len) + " symbols, its length says " + std::to_string(Y.dj[i].out_len));
                return AGC_HIP_EINVAL;
            }
    }
    // every segment has passed: from here on things are written
    CHK(ensure(c, c->rd.d_fa_sym, Y.sym_total + 64));
    uint8_t *d_sym = c->rd.d_fa_sym.as<uint8_t>();
    if (n_dj)
        CHK(decode_write(c, n_dj, d_sym));
    if (n_cj) {
        CHK(ensure(c, c->rd.d_fa_copy, (size_t)n_cj * sizeof(CopyJob)));
        CHK(upload(c, c->rd.d_fa_copy.p, Y.cj.data(), (size_t)n_cj * sizeof(CopyJob), c->stream));
        KTimer t(c, AGC_HIP_K_FASTA_OUT);
        hipLaunchKernelGGL(segment_copy_kernel, dim3((n_cj + 3) / 4), dim3(4 * WAVE), 0, c->stream, (const RefDesc *)c->d_refs.p, (const CopyJob *)c->rd.d_fa_copy.p, n_cj,
                           (const uint8_t *)c->rd.d_dec_enc.p, d_sym); // a wave per segment
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
        hipLaunchKernelGGL(fasta_text_kernel, dim3((uint32_t)text_blocks), dim3(256), 0, c->stream, P, d_text, a, Y.text, n_chunks);
    }
    HIPCHK(c, hipGetLastError());
    return hand_back(c, h_text, d_text, Y.text);
}

// The zstd decode.  The host reads every frame header: that sizes the output, and a frame whose header is refused never reaches the
// decoder.  zstd_decode_kernel then gives every other frame a wave, its slice of the output and its slice of the literals
// workspace (min(content size, 128 KiB): what a block's literals can need).
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
        const uint32_t ws_len = (std::min(h.contentSize, zs::BLOCKSIZE_MAX) + 15u) & ~15u;
        jobs[i] = {h_src_off[i] - s0, tot, ws_tot, (uint32_t)len, h.contentSize, ws_len, h.status};
        h_out_off[i] = tot;
        tot += h.contentSize;
        ws_tot += ws_len;
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
        CHK(ensure(c, c->rd.d_zd_jobs, (size_t)n * sizeof(ZDecJob)));
        CHK(ensure(c, c->rd.d_zd_status, (size_t)n * sizeof(uint32_t)));
        CHK(ensure(c, c->rd.d_zd_ws, ws_tot + 64));
        // (an output of 0 bytes: the context's buffer stands in for a d_out the caller did not have to give)
        CHK(output_buffer(c, d_out, c->rd.d_zd_out, tot));
        CHK(upload(c, c->rd.d_zd_src.p, h_src + s0, src_bytes, c->stream));
        CHK(upload(c, c->rd.d_zd_jobs.p, jobs.data(), (size_t)n * sizeof(ZDecJob), c->stream));
        {
            KTimer t(c, AGC_HIP_K_ZSTD_DECODE);
            hipLaunchKernelGGL(zstd_decode_kernel, dim3(n), dim3(WAVE), 0, c->stream, (const ZDecJob *)c->rd.d_zd_jobs.p, n, (const uint8_t *)c->rd.d_zd_src.p, d_out,
                               (uint8_t *)c->rd.d_zd_ws.p, (uint32_t *)c->rd.d_zd_status.p); // a wave per frame
        }
        HIPCHK(c, hipGetLastError());
        HIPCHK(c, hipMemcpyAsync(status.data(), c->rd.d_zd_status.p, (size_t)n * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
        CHK(hand_back(c, h_out, d_out, tot));
    } else
        for (uint32_t i = 0; i < n; ++i)
            status[i] = jobs[i].status;
    for (uint32_t i = 0; i < n; ++i)
        if (h_status)
            h_status[i] = status[i];
    for (uint32_t i = 0; i < n; ++i)
        if (status[i] != zs::dec::OK) {
            c->err = "zstd_decode: frame " + std::to_string(i) + " is refused: " + (status[i] == zs::dec::UNSUPPORTED ? "unsupported (status 1)" : "malformed (status 2)");
            return AGC_HIP_EINVAL;
        }
    return AGC_HIP_OK;
}

extern "C" {

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

} // extern "C"
