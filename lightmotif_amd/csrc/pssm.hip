// pssm.hip -- lm_hip_pssm_*: the device side of a ScoringMatrix (pwm/mod.rs:529-662).  All tables of a matrix are built
// on the host as one image (pssm_tables.hpp: which tables exist for a given (M, K), and what is in them) and live in ONE
// device allocation, lm_hip_pssm::d_slab; the d_* fields the launch code reads are views into it.
#include <new>

#include "pssm_tables.hpp"

using namespace lm;

extern "C" {

// ---- PSSM ---------------------------------------------------------------------------------

int lm_hip_pssm_create(lm_hip_ctx *ctx, const float *pssm, size_t m, size_t stride, size_t k,
                       lm_hip_pssm **out)
{
    if (!ctx || !out || (!pssm && m))
        return fail(LM_HIP_ERR_BAD_ARGS, "pssm_create: null argument");
    *out = nullptr;
    if (k == 0 || k > 256 || stride < k)
        return fail(LM_HIP_ERR_BAD_ARGS, "pssm_create: bad alphabet size %zu / stride %zu", k, stride);
    std::lock_guard<std::mutex> lock(ctx->mu);
    DeviceGuard guard(ctx->device);
    lm_hip_pssm *p = new (std::nothrow) lm_hip_pssm();
    if (!p)
        return fail(LM_HIP_ERR_OOM, "out of host memory");
    p->device = ctx->device;
    p->m = m;
    p->k = k;
    p->host.resize(m * k);
    for (size_t j = 0; j < m; ++j)
        for (size_t s = 0; s < k; ++s)
            p->host[j * k + s] = pssm[j * stride + s];
    const PssmTables t = build_pssm_tables(p->host.data(), m, k, ctx->xlong_store);
    if (!t.bytes.empty()) {
        hipError_t e = hipMalloc(&p->d_slab, t.bytes.size());
        if (e != hipSuccess) {
            lm_hip_pssm_destroy(p);
            return fail(LM_HIP_ERR_OOM, "hipMalloc(pssm) failed: %s", hipGetErrorString(e));
        }
        e = hipMemcpyAsync(p->d_slab, t.bytes.data(), t.bytes.size(), hipMemcpyHostToDevice, ctx->stream);
        if (e == hipSuccess)
            e = hipStreamSynchronize(ctx->stream);  // `t` dies with this scope
        if (e != hipSuccess) {
            lm_hip_pssm_destroy(p);
            return fail(LM_HIP_ERR_HIP, "pssm upload failed: %s", hipGetErrorString(e));
        }
    }
    auto floats = [&](size_t off) { return off == kAbsent ? nullptr : (float *)(p->d_slab + off); };
    auto dwords = [&](size_t off) { return off == kAbsent ? nullptr : (unsigned *)(p->d_slab + off); };
    p->d_dense = floats(t.dense);
    p->d_table = floats(t.table);
    p->d_table_pad = floats(t.table_pad);
    for (const auto &part : t.parts)
        p->parts.push_back({part.off, part.m, part.ts, part.lead, floats(part.table)});
    p->d_image = dwords(t.image);
    p->d_image2 = dwords(t.image2);
    p->d_image2_drop = dwords(t.image2_drop);
    p->d_image2_multi = dwords(t.image2_multi);
    p->ts = t.ts;
    p->lead = t.lead;
    p->drop_dmax = t.drop_dmax;
    p->has_prefilter = t.has_prefilter;
    p->pre_offset = t.pre_offset;
    p->pre_factor = t.pre_factor;
    p->pre_emax = t.pre_emax;
    *out = p;
    return LM_HIP_OK;
}

int lm_hip_pssm_reverse_complement(lm_hip_ctx *ctx, const lm_hip_pssm *pssm, lm_hip_pssm **out)
{
    if (!ctx || !pssm || !out)
        return fail(LM_HIP_ERR_BAD_ARGS, "pssm_reverse_complement: null argument");
    *out = nullptr;
    if (pssm->k != 5)
        return fail(LM_HIP_ERR_BAD_ARGS, "pssm_reverse_complement: only DNA matrices (K = 5) have a complement");
    static const int comp[5] = {2, 3, 0, 1, 4};  // A C T G N -> T G A C N
    const size_t m = pssm->m, k = pssm->k;
    std::vector<float> rc(m * k);
    for (size_t i = 0; i < m; ++i)  // pwm/mod.rs:570-574
        for (size_t s = 0; s < k; ++s)
            rc[i * k + s] = pssm->host[(m - 1 - i) * k + comp[s]];
    return lm_hip_pssm_create(ctx, rc.data(), m, k, k, out);
}

int lm_hip_pssm_destroy(lm_hip_pssm *p)
{
    if (!p)
        return LM_HIP_OK;
    DeviceGuard guard(p->device);
    if (p->d_slab)
        (void)hipFree(p->d_slab);  // every d_* field is a view into it
    delete p;
    return LM_HIP_OK;
}

size_t lm_hip_pssm_len(const lm_hip_pssm *p) { return p ? p->m : 0; }

}  // extern "C"
