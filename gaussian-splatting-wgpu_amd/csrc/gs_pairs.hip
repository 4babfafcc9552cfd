// gs_pairs.hip -- the pair moments' entry points: the exact sums over the matched pairs (p_i, p_partner[i]) of the resident splats
// that pass a state filter -- what a rigid or similarity fit needs --, and the same numbers from host planes.  Part of the C ABI
// (include/gsplat/gs_abi.h "registration"); the kernel is in k_pairs.hip, the pairing rule and the host loop in gs_pair_host.h, the
// arithmetic in gs_exact_sum.h.
//
// The reference has no counterpart: it is a viewer.  An editor on it would export both captures' 320-byte records, build a k-d tree
// and run ICP on the host; here a step's sums are 352 bytes after one streaming pass, and gsplat.register builds the fit on them.
//
// gs_pair_moments drains the context's ring first (gs_wait), runs on the context's stream and returns when done, as the moments do.
// It launches nothing in a frame: a context that never calls it launches exactly what it did before.
#include <cmath>

#include "gs_runtime.h"
#include "gs_pair_host.h"

static_assert(sizeof(struct gs_pair_moments) == 352 && offsetof(struct gs_pair_moments, sum_p) == 16 && offsetof(struct gs_pair_moments, pq) == 112 &&
                  offsetof(struct gs_pair_moments, pp) == 256 && offsetof(struct gs_pair_moments, qq) == 304,
              "gs_pair_moments layout");
static_assert(GS_PAIRS_SLOT_WORDS >= GS_PAIR_QUANTITIES * GS_EX_LIMBS + 2u, "a slot holds 21 limb tables and the two counts");

// The record from the 21 limb tables in gs_pair_host.h's order, which is the record's own: each sum finished once.
static void pairs_finish(const int64_t* tables, uint64_t matched, uint64_t paired, struct gs_pair_moments* out) {
    memset(out, 0, sizeof(*out));
    out->matched = matched;
    out->paired = paired;
    gs_exact* e = out->sum_p; // sum_p, sum_q, pq, pp, qq are contiguous (the layout is asserted above)
    for (uint32_t t = 0; t < GS_PAIR_QUANTITIES; ++t) ex_finish(tables + (size_t)t * GS_EX_LIMBS, &e[t].hi, &e[t].lo);
}

static int32_t pairs_check_dist(const char* who, float max_dist2) {
    if (!(max_dist2 >= 0.0f)) return fail(GS_ERR_INVALID_ARGUMENT, "%s: max_dist2 %g is negative or NaN", who, (double)max_dist2);
    return GS_OK;
}

GS_EXPORT int32_t gs_pair_moments(gs_ctx* c, uint32_t mask, uint32_t value, const uint32_t* partner, float max_dist2, struct gs_pair_moments* out) {
    static const char* who = "gs_pair_moments";
    int32_t rc = resident_check(c, who, Plane::filtered, mask, value);
    if (rc != GS_OK) return rc;
    rc = pairs_check_dist(who, max_dist2);
    if (rc != GS_OK) return rc;
    if (!out) return fail(GS_ERR_INVALID_ARGUMENT, "%s: null moments", who);
    if (c->n >= 0x80000000u) return fail(GS_ERR_INVALID_ARGUMENT, "%s: %llu splats, a limb holds fewer than 2^31 terms", who, (unsigned long long)c->n);
    rc = resident_drain(c);
    if (rc != GS_OK) return rc;
    const uint8_t* state = (mask | value) ? c->scene.state : nullptr;
    constexpr size_t kWords = (size_t)GS_PAIRS_SLOTS * GS_PAIRS_SLOT_WORDS;
    std::vector<unsigned long long> h(kWords, 0ull);
    if (c->n) {
        const uint32_t* ids;
        if (partner) { // a host array: to the context's scratch first
            rc = c->pr.partner.reserve(((uint64_t)c->n + 3u) & ~3ull);
            if (rc != GS_OK) return rc;
            HIP_TRY(hipMemcpyAsync(c->pr.partner, partner, (size_t)c->n * 4, hipMemcpyHostToDevice, c->stream));
            ids = c->pr.partner;
        } else { // the context's own nearest plane, in place: GS_KNN_NONE everywhere when it was never searched or has been dropped
            rc = knn_planes(c, c->stream);
            if (rc != GS_OK) return rc;
            ids = c->kn.nearest;
        }
        if (!c->pr.slots) HIP_TRY(hipMalloc(c->pr.slots.out(), kWords * 8));
        HIP_TRY(hipMemsetAsync(c->pr.slots, 0, kWords * 8, c->stream));
        gs_launch_pairs(state, c->scene.px, c->scene.py, c->scene.pz, ids, c->n, mask, value, max_dist2, c->pr.slots, c->opt.grid_persist, c->stream);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpyAsync(h.data(), c->pr.slots, kWords * 8, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(hipStreamSynchronize(c->stream));
    }
    // the copies add up in wrapping unsigned arithmetic; the totals are within i64 (gs_exact_sum.h)
    constexpr uint32_t words = GS_PAIR_QUANTITIES * GS_EX_LIMBS + 2u;
    int64_t total[words] = {};
    for (uint32_t s = 0; s < GS_PAIRS_SLOTS; ++s)
        for (uint32_t i = 0; i < words; ++i) total[i] = (int64_t)((uint64_t)total[i] + (uint64_t)h[(size_t)s * GS_PAIRS_SLOT_WORDS + i]);
    pairs_finish(total, (uint64_t)total[words - 2u], (uint64_t)total[words - 1u], out);
    return GS_OK;
}

GS_EXPORT int32_t gs_pair_moments_host(const float* px, const float* py, const float* pz, uint64_t n, const uint32_t* partner, const uint8_t* state,
                                       uint32_t mask, uint32_t value, float max_dist2, struct gs_pair_moments* out) {
    static const char* who = "gs_pair_moments_host";
    if ((!px || !py || !pz) && n) return fail(GS_ERR_INVALID_ARGUMENT, "%s: null position plane", who);
    if (!partner && n) return fail(GS_ERR_INVALID_ARGUMENT, "%s: null partner", who);
    if (mask > 0xFFu || value > 0xFFu) return fail(GS_ERR_INVALID_ARGUMENT, "%s: filter (0x%x, 0x%x) does not fit the state byte", who, mask, value);
    if ((mask | value) && !state && n) return fail(GS_ERR_INVALID_ARGUMENT, "%s: null state with the filter (0x%x, 0x%x)", who, mask, value);
    const int32_t rc = pairs_check_dist(who, max_dist2);
    if (rc != GS_OK) return rc;
    if (!out) return fail(GS_ERR_INVALID_ARGUMENT, "%s: null moments", who);
    if (n >= 0x80000000ull) return fail(GS_ERR_INVALID_ARGUMENT, "%s: %llu splats, a limb holds fewer than 2^31 terms", who, (unsigned long long)n);
    PairSums s;
    pair_sums_clear(&s);
    for (uint64_t i = 0; i < n; ++i) pair_host_one(&s, px, py, pz, n, partner, state, mask, value, max_dist2, i);
    pairs_finish(s.t, s.matched, s.paired, out);
    return GS_OK;
}
