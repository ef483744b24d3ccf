// statmc_score_sum_args.h -- what statmc_score_sum (include/statmc.h) checks and fills on the host, each rule stated once, the
// workspace layout, the argument block its kernels take (statmc_score_sum.hip) and the finalisation: 64-bit limb accumulators to the
// nearest double, in integers alone.  Pure functions of their arguments: no HIP call, no device, no global or thread-local state;
// nothing is read through a device pointer (the image pointers are compared as numbers; `caps` is a host array and is read).  The
// key, the message buffer and the pointer helpers are statmc_select_args.h's.  The finalisation is written once for host and device
// (STATMC_SUM_HD is empty without hipcc): tests/cpp/test_score_sum_args.cpp compiles this header with nothing but include/statmc.h,
// with and without sanitizers, and holds it to a long division of its own.
#pragma once

#include "statmc_select_args.h"

#if defined(__HIPCC__)
#define STATMC_SUM_HD __host__ __device__
#else
#define STATMC_SUM_HD
#endif

namespace statmc {

// ---- the value of a key 0 < k < 0x7F800000 as an integer: val(k) = M * 2^(s - 149), M < 2^24, s <= 253
STATMC_SUM_HD inline uint32_t sum_significand(uint32_t k) { return (k >> 23) ? ((k & 0x7FFFFFu) | 0x800000u) : (k & 0x7FFFFFu); }
STATMC_SUM_HD inline int sum_shift(uint32_t k) { return (k >> 23) ? (int)(k >> 23) - 1 : 0; }
constexpr uint32_t kSumInfinite = 0x7F800000u;
constexpr int kSumUnitExp = -149, kSumSqUnitExp = -298;   // the unit of the sums' integers, of the squares'

// ---- the fixed-point integers: limb l holds the bits 32 l .. 32 l + 31, in a 64-bit word so that 2^32 pixels of
// less than 2^32 each cannot overflow it.  M << (s & 31) lands in limbs s >> 5 and the next (s >> 5 <= 7); M^2 << (2 s & 31) in
// limbs 2 s >> 5 and the next two (2 s >> 5 <= 15).
constexpr int kSumLimbs = 10, kSumSqLimbs = 19;
constexpr int kSumIntervals = STATMC_SUM_MAX_CAPS + 1;   // of the finite non-zero keys, between the sorted caps: a pixel's is the number of caps below its key
static_assert(kSumLimbs > (253 >> 5) + 1 && kSumSqLimbs > (506 >> 5) + 2, "the largest finite key lands inside");
static_assert(kSumLimbs * 32 >= 277 + 32 && kSumSqLimbs * 32 >= 554 + 32, "2^32 pixels at the largest finite key fit");

// the workspace, in 64-bit words: the class counts, the intervals' pixel counts, their sum limbs, their square limbs
enum {
    kSumWsZero = 0, kSumWsInfinite = 1, kSumWsCount = 2, kSumWsSum = 8, kSumWsSq = kSumWsSum + kSumIntervals * kSumLimbs,
    kSumWsUsed = kSumWsSq + kSumIntervals * kSumSqLimbs, kSumWsWords = (kSumWsUsed + 7) / 8 * 8
};
static_assert(kSumWsCount + kSumIntervals <= kSumWsSum, "the counts end before the limbs");
inline size_t sum_workspace_bytes() { return (size_t)kSumWsWords * sizeof(uint64_t); }

struct SumArgs {
    const float *score;
    statmc_sum_result *result;
    unsigned long long *ws;
    long long n_px, n_chunks;
    uint32_t cap_key[STATMC_SUM_MAX_CAPS];   // as asked
    uint32_t sorted[STATMC_SUM_MAX_CAPS];    // ascending; entries n_caps .. 3 are 0xFFFFFFFF: no key is above them
    int under[STATMC_SUM_MAX_CAPS];          // the number of sorted caps <= cap_key[j]: the intervals 0 .. under[j] - 1 lie at or below cap j
    int n_caps;
    int grid;
    int vec;
};

// statmc_score_sum, in this order: the film size, NULL pointers, alignment, n_caps, NaN caps, the workspace size, result over the
// score image or the workspace, the workspace over the score image.
inline bool check_sum_call(uint16_t width, uint16_t height, const float *score, const float *caps, int n_caps, const statmc_sum_result *result,
                           const void *workspace, size_t workspace_bytes, SelectMsg m) {
    if (width == 0 || height == 0) return select_refuse(m, "empty image: width and height must be positive");
    if (!score) return select_refuse(m, "null score");
    if (!result) return select_refuse(m, "null result");
    if (!caps) return select_refuse(m, "null caps");
    if (!workspace) return select_refuse(m, "null workspace");
    if (select_misaligned(score, 4)) return select_refuse(m, "score is not 4-byte aligned");
    if (select_misaligned(result, 8)) return select_refuse(m, "result is not 8-byte aligned");
    if (select_misaligned(workspace, 8)) return select_refuse(m, "workspace is not 8-byte aligned");
    if (n_caps < 1 || n_caps > STATMC_SUM_MAX_CAPS) return select_refuse(m, "n_caps = %d: 1 to %d", n_caps, STATMC_SUM_MAX_CAPS);
    for (int i = 0; i < n_caps; i++)
        if ((select_float_bits(caps[i]) & 0x7FFFFFFFu) > 0x7F800000u) return select_refuse(m, "caps[%d] is NaN", i);
    const size_t need = sum_workspace_bytes();
    if (workspace_bytes < need)
        return select_refuse(m, "workspace_bytes = %zu: statmc_score_sum_workspace asks for %zu", workspace_bytes, need);
    const size_t px = (size_t)width * height * 4;
    if (select_ranges_overlap(result, sizeof(statmc_sum_result), score, px)) return select_refuse(m, "result overlaps score");
    if (select_ranges_overlap(result, sizeof(statmc_sum_result), workspace, need)) return select_refuse(m, "result overlaps workspace");
    if (select_ranges_overlap(workspace, need, score, px)) return select_refuse(m, "workspace overlaps score");
    return true;
}

// The kernels' argument block of a call that passed check_sum_call.
inline void fill_sum_args(SumArgs &a, uint16_t width, uint16_t height, const float *score, const float *caps, int n_caps,
                          statmc_sum_result *result, void *workspace) {
    a = SumArgs{};
    a.score = score, a.result = result;
    a.ws = static_cast<unsigned long long *>(workspace);
    a.n_px = (long long)width * height;
    a.n_chunks = select_chunks(width, height);
    a.n_caps = n_caps;
    for (int i = 0; i < STATMC_SUM_MAX_CAPS; i++) {
        a.cap_key[i] = i < n_caps ? select_key(select_float_bits(caps[i])) : 0u;
        a.sorted[i] = i < n_caps ? a.cap_key[i] : 0xFFFFFFFFu;
    }
    for (int i = 1; i < STATMC_SUM_MAX_CAPS; i++)      // insertion sort of four
        for (int j = i; j > 0 && a.sorted[j - 1] > a.sorted[j]; j--) {
            const uint32_t t = a.sorted[j];
            a.sorted[j] = a.sorted[j - 1], a.sorted[j - 1] = t;
        }
    for (int j = 0; j < STATMC_SUM_MAX_CAPS; j++) {
        a.under[j] = 0;
        for (int i = 0; i < n_caps; i++) a.under[j] += j < n_caps && a.sorted[i] <= a.cap_key[j];
    }
    a.grid = (int)(a.n_chunks < kSelectMaxGrid ? a.n_chunks : kSelectMaxGrid);
    a.vec = !select_misaligned(score, 16);
}

// ---------------------------------------------------------------- the finalisation: integers only
// acc[0 .. n): 64-bit accumulators of 32-bit limbs, any values.  limb[0 .. n + 2): the same integer, every limb below 2^32.
STATMC_SUM_HD inline void sum_carry(const uint64_t *acc, int n, uint32_t *limb) {
    uint64_t carry = 0;   // below 2^33
    for (int i = 0; i < n; i++) {
        const uint64_t t = carry + (acc[i] & 0xFFFFFFFFull);
        limb[i] = (uint32_t)t;
        carry = (t >> 32) + (acc[i] >> 32);
    }
    limb[n] = (uint32_t)carry;
    limb[n + 1] = (uint32_t)(carry >> 32);
}

// limb[0 .. n) += count * v[0 .. nv) * 2^(32 at); the caller's bound keeps the total inside the n limbs (a carry out of them is dropped)
STATMC_SUM_HD inline void sum_add_product(uint32_t *limb, int n, int at, const uint32_t *v, int nv, uint32_t count) {
    uint64_t carry = 0;
    int k = at;
    for (int i = 0; i < nv && k < n; i++, k++) {
        const uint64_t t = (uint64_t)v[i] * count + limb[k] + carry;   // at most (2^32 - 1)^2 + 2 (2^32 - 1) = 2^64 - 1
        limb[k] = (uint32_t)t;
        carry = t >> 32;
    }
    for (; carry && k < n; k++) {
        const uint64_t t = (uint64_t)limb[k] + carry;
        limb[k] = (uint32_t)t;
        carry = t >> 32;
    }
}

// The bits of the double nearest, ties to even, to N * 2^unit_exp, N the integer of limb[0 .. n).  N = 0 gives +0; the result of a
// non-zero N must be a normal double (statmc_score_sum's lie in [2^-298, 2^288)).
STATMC_SUM_HD inline uint64_t sum_round_bits(const uint32_t *limb, int n, int unit_exp) {
    int top = n - 1;
    while (top >= 0 && limb[top] == 0) top--;
    if (top < 0) return 0;
    int hb = 31;
    while (!((limb[top] >> hb) & 1u)) hb--;
    hb += 32 * top;   // N's highest set bit
    uint64_t mant = 0;   // bits hb .. hb - 52 of N (bits below 0 are 0)
    for (int b = 0; b < 53; b++) {
        const int at = hb - b;
        const uint64_t bit = at >= 0 ? (limb[at >> 5] >> (at & 31)) & 1u : 0u;
        mant = (mant << 1) | bit;
    }
    if (hb >= 53) {
        const int r = hb - 53;   // the round bit
        const bool half = (limb[r >> 5] >> (r & 31)) & 1u;
        bool sticky = false;
        for (int i = 0; i < (r >> 5); i++) sticky |= limb[i] != 0;
        if (r & 31) sticky |= (limb[r >> 5] & ((1u << (r & 31)) - 1u)) != 0;
        if (half && (sticky || (mant & 1u))) mant++;
        if (mant >> 53) mant >>= 1, hb++;
    }
    return ((uint64_t)(hb + unit_exp + 1023) << 52) | (mant & 0xFFFFFFFFFFFFFull);
}

// accumulators to the nearest double's bits, in one step
STATMC_SUM_HD inline uint64_t sum_limbs_to_double_bits(const uint64_t *acc, int n, int unit_exp) {
    uint32_t limb[kSumSqLimbs + 2];   // n <= kSumSqLimbs
    sum_carry(acc, n, limb);
    return sum_round_bits(limb, n + 2, unit_exp);
}

// One cap's slot from the totals of the workspace: the intervals at or below the cap, plus the pixels above it at the cap's value.
// ws is the workspace as the pass left it; key is the cap's, under the number of sorted caps <= key (SumArgs::under).
STATMC_SUM_HD inline void sum_finalize_slot(const uint64_t *ws, uint32_t key, int under, int64_t *n_clipped, uint64_t *sum_bits, uint64_t *sq_bits) {
    uint64_t clipped = key < kSumInfinite ? ws[kSumWsInfinite] : 0;
    for (int t = under; t < kSumIntervals; t++) clipped += ws[kSumWsCount + t];
    uint64_t acc[kSumSqLimbs];
    uint32_t limb[kSumSqLimbs + 2];
    const bool at_cap = key > 0 && key < kSumInfinite && clipped != 0;   // (clipped < 2^32: a film has fewer pixels)
    const uint32_t M = sum_significand(key);
    const int s = sum_shift(key);

    for (int l = 0; l < kSumLimbs; l++) {
        acc[l] = 0;
        for (int t = 0; t < under; t++) acc[l] += ws[kSumWsSum + t * kSumLimbs + l];   // all of a film's pixels: below 2^64
    }
    sum_carry(acc, kSumLimbs, limb);
    if (at_cap) {
        const uint64_t v = (uint64_t)M << (s & 31);
        const uint32_t v32[2] = {(uint32_t)v, (uint32_t)(v >> 32)};
        sum_add_product(limb, kSumLimbs + 2, s >> 5, v32, 2, (uint32_t)clipped);
    }
    *sum_bits = sum_round_bits(limb, kSumLimbs + 2, kSumUnitExp);

    for (int l = 0; l < kSumSqLimbs; l++) {
        acc[l] = 0;
        for (int t = 0; t < under; t++) acc[l] += ws[kSumWsSq + t * kSumSqLimbs + l];
    }
    sum_carry(acc, kSumSqLimbs, limb);
    if (at_cap) {
        const uint64_t q = (uint64_t)M * M;   // below 2^48
        const int sh = (2 * s) & 31;
        const uint64_t upper = q >> (32 - sh);   // a shift of 1 .. 32
        const uint32_t v32[3] = {(uint32_t)(q << sh), (uint32_t)upper, (uint32_t)(upper >> 32)};
        sum_add_product(limb, kSumSqLimbs + 2, (2 * s) >> 5, v32, 3, (uint32_t)clipped);
    }
    *sq_bits = sum_round_bits(limb, kSumSqLimbs + 2, kSumSqUnitExp);
    *n_clipped = (int64_t)clipped;
}

}  // namespace statmc
