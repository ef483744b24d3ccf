// statmc_score_sum_args.h on its own: no library, no device, nothing but include/statmc.h.
//
// 1. The finalisation (sum_limbs_to_double_bits), always, against a big-integer long division written here: hand-made accumulators
//    with carries across every limb, exact ties of both parities, the smallest and the largest totals, 1000 random sets.  Any
//    difference ends the program with status 1.
// 2. A table of lines -- the one tests/test_score_sum_cpu.py writes from its restatement of include/statmc.h:
//      sum <name> <width> <height>  <score result workspace> <workspace_bytes>  <caps given: 0 / 1> <n_caps> <k> <k caps as float bits>
//      slot <name> <k> <k pixels as float bits> <n_caps> <n_caps caps as float bits>
//    The image "pointers" of a sum line are numbers: nothing is read through them.  A slot line is the whole computation on the host:
//    the pixels are added into a workspace as the pass defines it, sum_finalize_slot does the rest.
// Output, one line per entry:   <name> : ok sum <workspace bytes> <chunks> <grid> <vec> <cap keys, 8 hex digits> / <sorted> / <under>   |
//                               <name> : slot <n_zero> <n_finite> <n_infinite> then per cap <n_clipped> <sum bits> <sum_sq bits> (16 hex digits)   |
//                               <name> : <message>
#include <inttypes.h>
#include <stdio.h>
#include <string.h>

#include <vector>

#include "../../statmc_amd/csrc/statmc_score_sum_args.h"

template <typename T>
static T *at(uint64_t address) { return reinterpret_cast<T *>((uintptr_t)address); }

// ---------------------------------------------------------------- a big integer of bits, the simple way
typedef std::vector<uint8_t> Big;   // one bit per entry, least significant first
static Big big_of_words(const uint64_t *acc, int n) {   // sum of acc[i] * 2^(32 i)
    Big b((size_t)(32 * n + 80), 0);
    for (int i = 0; i < n; i++) {
        int carry = 0;
        for (size_t k = 0; k + 32 * (size_t)i < b.size(); k++) {
            const int add = k < 64 ? (int)((acc[i] >> k) & 1u) : 0;
            if (k >= 64 && !carry) break;
            const int t = b[32 * (size_t)i + k] + add + carry;
            b[32 * (size_t)i + k] = (uint8_t)(t & 1), carry = t >> 1;
        }
    }
    return b;
}
static int big_top(const Big &b) {
    for (int i = (int)b.size() - 1; i >= 0; i--)
        if (b[(size_t)i]) return i;
    return -1;
}
static int big_cmp(const Big &a, const Big &b) {
    for (int i = (int)(a.size() > b.size() ? a.size() : b.size()) - 1; i >= 0; i--) {
        const int x = (size_t)i < a.size() ? a[(size_t)i] : 0, y = (size_t)i < b.size() ? b[(size_t)i] : 0;
        if (x != y) return x < y ? -1 : 1;
    }
    return 0;
}
static void big_sub(Big &a, const Big &b) {   // a -= b, a >= b
    int borrow = 0;
    for (size_t i = 0; i < a.size(); i++) {
        const int t = a[i] - (i < b.size() ? b[i] : 0) - borrow;
        a[i] = (uint8_t)(t & 1), borrow = t < 0;
    }
}
// schoolbook long division, a bit of the dividend at a time: q = n / d, r = n % d
static void big_divmod(const Big &n, const Big &d, Big &q, Big &r) {
    q.assign(n.size(), 0);
    r.assign(d.size() + 1, 0);
    for (int i = (int)n.size() - 1; i >= 0; i--) {
        r.insert(r.begin(), n[(size_t)i]);
        r.pop_back();
        if (big_cmp(r, d) >= 0) big_sub(r, d), q[(size_t)i] = 1;
    }
}
// the bits of the double nearest, ties to even, to n * 2^unit_exp
static uint64_t big_round(const Big &n, int unit_exp) {
    int hb = big_top(n);
    if (hb < 0) return 0;
    uint64_t mant = 0;
    if (hb <= 52) {
        for (int i = hb; i >= 0; i--) mant = (mant << 1) | n[(size_t)i];
        mant <<= 52 - hb;
    } else {
        Big d((size_t)(hb - 52) + 1, 0), q, r, twice;
        d.back() = 1;   // 2^(hb - 52): the quotient has 53 bits
        big_divmod(n, d, q, r);
        for (int i = 52; i >= 0; i--) mant = (mant << 1) | q[(size_t)i];
        twice = r;
        twice.insert(twice.begin(), 0);
        const int c = big_cmp(twice, d);
        if (c > 0 || (c == 0 && (mant & 1u))) mant++;
        if (mant >> 53) mant >>= 1, hb++;
    }
    return ((uint64_t)(hb + unit_exp + 1023) << 52) | (mant & 0xFFFFFFFFFFFFFull);
}

static int n_checked = 0;
static bool check(const char *what, const uint64_t *acc, int n, int unit_exp) {
    const uint64_t got = statmc::sum_limbs_to_double_bits(acc, n, unit_exp), want = big_round(big_of_words(acc, n), unit_exp);
    n_checked++;
    if (got == want) return true;
    fprintf(stderr, "%s: %016" PRIx64 ", the long division gives %016" PRIx64 "\n", what, got, want);
    return false;
}
static bool check_is(const char *what, const uint64_t *acc, int n, int unit_exp, double want) {
    uint64_t bits;
    memcpy(&bits, &want, sizeof(bits));
    const uint64_t got = statmc::sum_limbs_to_double_bits(acc, n, unit_exp);
    if (got != bits) fprintf(stderr, "%s: %016" PRIx64 ", expected %016" PRIx64 "\n", what, got, bits);
    return check(what, acc, n, unit_exp) && got == bits;
}

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;   // splitmix64, fixed seed
static uint64_t rng() {
    uint64_t z = (rng_state += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

static bool finalisation() {
    using namespace statmc;
    bool ok = true;
    uint64_t acc[kSumSqLimbs];
    const int sizes[2] = {kSumLimbs, kSumSqLimbs}, units[2] = {kSumUnitExp, kSumSqUnitExp};
    for (int which = 0; which < 2; which++) {
        const int n = sizes[which], unit = units[which];
        // zero, the smallest total, the smallest normal-looking ones
        for (int i = 0; i < n; i++) acc[i] = 0;
        ok &= statmc::sum_limbs_to_double_bits(acc, n, unit) == 0;
        acc[0] = 1;
        ok &= check_is("the smallest total", acc, n, unit, which ? 0x1p-298 : 0x1p-149);
        acc[0] = 3;
        ok &= check_is("three units", acc, n, unit, which ? 0x3p-298 : 0x3p-149);
        // carries across every limb: every accumulator full
        for (int i = 0; i < n; i++) acc[i] = ~0ull;
        ok &= check("every accumulator full", acc, n, unit);
        // ... and a carry that ripples: 2^32 - 1 in every limb, one more unit at the bottom
        for (int i = 0; i < n; i++) acc[i] = 0xFFFFFFFFull;
        acc[0] += 1;
        ok &= check("a carry through every limb", acc, n, unit);
        for (int i = 0; i < n; i++) acc[i] = 0xFFFFFFFFull;
        ok &= check("all ones rounds up to a power of two", acc, n, unit);
        // exact ties, both parities, at every limb offset: 2^53 + 1 (ties down to even) and 2^53 + 3 (ties up to even), times 2^(32 l + k)
        for (int l = 0; l + 2 < n; l++)
            for (int k = 0; k < 32; k += 7) {
                for (int parity = 0; parity < 2; parity++) {
                    for (int i = 0; i < n; i++) acc[i] = 0;
                    const uint64_t v = (1ull << 53) + (parity ? 3 : 1);   // 54 bits: spread over limbs l, l + 1, l + 2 through the accumulators
                    acc[l] = (v << k) & 0xFFFFFFFFull;
                    acc[l + 1] = (k ? v >> (32 - k) : v >> 32);   // up to 54 bits in one accumulator: carries into l + 2
                    const uint64_t got = statmc::sum_limbs_to_double_bits(acc, n, unit);
                    const double want = (parity ? 0x1.0000000000002p53 : 0x1p53) * (which ? 0x1p-298 : 0x1p-149);
                    double scaled = want;
                    for (int s = 0; s < 32 * l + k; s++) scaled *= 2;
                    uint64_t bits;
                    memcpy(&bits, &scaled, sizeof(bits));
                    if (got != bits) fprintf(stderr, "tie at limb %d bit %d parity %d: %016" PRIx64 " expected %016" PRIx64 "\n", l, k, parity, got, bits), ok = false;
                    ok &= check("a tie", acc, n, unit);
                    acc[0] |= l || k ? 1u : 0u;   // one unit far below breaks the tie upwards
                    if (l || k) ok &= check("a broken tie", acc, n, unit);
                }
            }
    }
    // the largest totals: every pixel of a 65535 x 65535 film at the maximum finite key, as the pass adds them
    {
        const uint64_t px = 65535ull * 65535ull, M = 0xFFFFFF;
        const int s = 253;
        for (int i = 0; i < kSumSqLimbs; i++) acc[i] = 0;
        const uint64_t v = M << (s & 31);
        acc[s >> 5] = (v & 0xFFFFFFFFull) * px, acc[(s >> 5) + 1] = (v >> 32) * px;
        ok &= check("the largest sum", acc, kSumLimbs, kSumUnitExp);
        for (int i = 0; i < kSumSqLimbs; i++) acc[i] = 0;
        const uint64_t q = M * M, upper = q >> (32 - ((2 * s) & 31));
        acc[(2 * s) >> 5] = ((q << ((2 * s) & 31)) & 0xFFFFFFFFull) * px;
        acc[((2 * s) >> 5) + 1] = (upper & 0xFFFFFFFFull) * px, acc[((2 * s) >> 5) + 2] = (upper >> 32) * px;
        ok &= check("the largest sum of squares", acc, kSumSqLimbs, kSumSqUnitExp);
        const uint64_t top = statmc::sum_limbs_to_double_bits(acc, kSumSqLimbs, kSumSqUnitExp);
        ok &= (int)(top >> 52) - 1023 < 288;
    }
    // random accumulators: full words, sparse words, short totals
    for (int it = 0; it < 1000; it++) {
        const int which = it & 1, n = sizes[which];
        const int used = 1 + (int)(rng() % (uint64_t)n);
        for (int i = 0; i < n; i++) {
            uint64_t w = i < used ? rng() : 0;
            if (it % 3 == 1) w >>= rng() % 64;
            if (it % 5 == 2 && (rng() & 1)) w = 0;
            if (it % 7 == 3) w = (rng() & 1) ? ~0ull : 0xFFFFFFFFull;
            acc[i] = w;
        }
        if (it % 11 == 4) acc[0] = 0, acc[used - 1] |= 1ull << 63;   // a long run of zeros below
        ok &= check("random accumulators", acc, n, units[which]);
    }
    return ok;
}

int main(int argc, char **argv) {
    if (argc != 2) {
        fprintf(stderr, "usage: %s <table>\n", argv[0]);
        return 2;
    }
    if (statmc::sum_workspace_bytes() != statmc::sum_workspace_bytes() || statmc::sum_workspace_bytes() % 8 != 0 ||
        statmc::sum_workspace_bytes() < (size_t)statmc::kSumWsUsed * 8) {
        fprintf(stderr, "the workspace helper is not a pure multiple of 8 that holds the layout\n");
        return 2;
    }
    if (!finalisation()) return 1;
    FILE *f = fopen(argv[1], "r");
    if (!f) {
        perror(argv[1]);
        return 2;
    }
    printf("finalisation : ok %d\n", n_checked);
    char word[64], name[128], why[512];
    int n_calls = 0;
    while (fscanf(f, "%63s", word) == 1) {
        why[0] = 0;
        if (strcmp(word, "sum") == 0) {
            int width, height, given, n, k;
            uint64_t p[3], ws_bytes;
            if (fscanf(f, "%127s %d %d %" SCNu64 " %" SCNu64 " %" SCNu64 " %" SCNu64 " %d %d %d", name, &width, &height, &p[0], &p[1], &p[2], &ws_bytes,
                       &given, &n, &k) != 10 || k < 0 || k > 64) {
                fprintf(stderr, "bad sum line\n");
                return 2;
            }
            std::vector<float> caps((size_t)(k > 4 ? k : 4), 0.0f);
            for (int i = 0; i < k; i++) {
                uint32_t b;
                if (fscanf(f, "%" SCNu32, &b) != 1) return 2;
                memcpy(&caps[(size_t)i], &b, sizeof(b));
            }
            const float *cp = given ? caps.data() : nullptr;
            if (!statmc::check_sum_call((uint16_t)width, (uint16_t)height, at<float>(p[0]), cp, n, at<statmc_sum_result>(p[1]), at<void>(p[2]),
                                        (size_t)ws_bytes, statmc::SelectMsg{why, sizeof(why)})) {
                printf("%s : %s\n", name, why);
            } else {
                statmc::SumArgs a;
                statmc::fill_sum_args(a, (uint16_t)width, (uint16_t)height, at<float>(p[0]), cp, n, at<statmc_sum_result>(p[1]), at<void>(p[2]));
                printf("%s : ok sum %zu %lld %d %d", name, statmc::sum_workspace_bytes(), a.n_chunks, a.grid, a.vec);
                for (int i = 0; i < a.n_caps; i++) printf(" %08x", (unsigned)a.cap_key[i]);
                printf(" /");
                for (int i = 0; i < a.n_caps; i++) printf(" %08x", (unsigned)a.sorted[i]);
                printf(" /");
                for (int i = 0; i < a.n_caps; i++) printf(" %d", a.under[i]);
                printf("\n");
            }
        } else if (strcmp(word, "slot") == 0) {
            int k, n;
            if (fscanf(f, "%127s %d", name, &k) != 2 || k < 0 || k > (1 << 20)) return 2;
            std::vector<uint32_t> px((size_t)k);
            for (int i = 0; i < k; i++)
                if (fscanf(f, "%" SCNu32, &px[(size_t)i]) != 1) return 2;
            if (fscanf(f, "%d", &n) != 1 || n < 1 || n > STATMC_SUM_MAX_CAPS) return 2;
            float caps[STATMC_SUM_MAX_CAPS] = {0, 0, 0, 0};
            for (int i = 0; i < n; i++) {
                uint32_t b;
                if (fscanf(f, "%" SCNu32, &b) != 1) return 2;
                memcpy(&caps[i], &b, sizeof(b));
            }
            using namespace statmc;
            SumArgs a;
            fill_sum_args(a, 1, 1, at<float>(16), caps, n, at<statmc_sum_result>(4096), at<void>(8192));
            std::vector<uint64_t> ws((size_t)kSumWsWords, 0);
            for (uint32_t b : px) {   // the pass, a pixel at a time
                const uint32_t key = select_key(b);
                if (key == 0) { ws[kSumWsZero]++; continue; }
                if (key == kSumInfinite) { ws[kSumWsInfinite]++; continue; }
                int t = 0;
                for (int j = 0; j < STATMC_SUM_MAX_CAPS; j++) t += key > a.sorted[j];
                ws[(size_t)(kSumWsCount + t)]++;
                const uint64_t M = sum_significand(key);
                const int s = sum_shift(key), sh = (2 * s) & 31;
                const uint64_t v = M << (s & 31), q = M * M, upper = q >> (32 - sh);
                uint64_t *sum = &ws[(size_t)(kSumWsSum + t * kSumLimbs + (s >> 5))], *sq = &ws[(size_t)(kSumWsSq + t * kSumSqLimbs + ((2 * s) >> 5))];
                sum[0] += (uint32_t)v, sum[1] += v >> 32;
                sq[0] += (uint32_t)(q << sh), sq[1] += (uint32_t)upper, sq[2] += upper >> 32;
            }
            uint64_t finite = 0;
            for (int t = 0; t < kSumIntervals; t++) finite += ws[(size_t)(kSumWsCount + t)];
            printf("%s : slot %" PRIu64 " %" PRIu64 " %" PRIu64, name, ws[kSumWsZero], finite, ws[kSumWsInfinite]);
            for (int j = 0; j < n; j++) {
                int64_t clipped;
                uint64_t sum_bits, sq_bits;
                sum_finalize_slot(ws.data(), a.cap_key[j], a.under[j], &clipped, &sum_bits, &sq_bits);
                printf(" %" PRId64 " %016" PRIx64 " %016" PRIx64, clipped, sum_bits, sq_bits);
            }
            printf("\n");
        } else {
            fprintf(stderr, "bad table near '%s'\n", word);
            return 2;
        }
        n_calls++;
    }
    fclose(f);
    return n_calls > 0 ? 0 : 2;
}
