// statmc_score_tiles_args.h on its own: no library, no device, nothing but include/statmc.h.
//
// 1. tile_mean_bits, always, against a bit-serial long division written here on one bit per byte: quotients on either side of 2^23
//    and 2^24, exact ties of both parities with a zero and a non-zero remainder, the divisors 1, 2, 3, 4095 and 4096, the smallest
//    total (one unit over 4096 pixels: +0), the largest (4096 pixels of the largest finite float), 1000 random totals.  Any
//    difference ends the program with status 1.
// 2. A table of lines -- the one tests/test_score_tiles_cpu.py writes from its restatement of include/statmc.h:
//      tiles <name> <width> <height> <score> <tile> <cap as float bits> <out given: 0 / 1> <sum sum_sq mean max n_px n_zero n_infinite n_clipped>
//      film <name> <width> <height> <tile> <cap as float bits> <width * height pixels as float bits>
//    The "pointers" of a tiles line are numbers: nothing is read through them.  A film line is the whole computation on the host: a
//    tile's pixels are added into a table as the kernel defines it, tile_capped_limbs, sum_round_bits and tile_mean_bits do the rest.
// Output, one line per entry:   <name> : ok tiles <tiles_x> <tiles_y> <n_tiles> <cap key, 8 hex digits> <vec>   |
//                               <name> : film <tiles_x> <tiles_y> then per tile, row-major,
//                                        <n_px> <n_zero> <n_infinite> <n_clipped> <sum bits> <sum_sq bits> <mean bits> <max bits> (hex)   |
//                               <name> : <message>
#include <inttypes.h>
#include <stdio.h>
#include <string.h>

#include <vector>

#include "../../statmc_amd/csrc/statmc_score_tiles_args.h"

template <typename T>
static T *at(uint64_t address) { return reinterpret_cast<T *>((uintptr_t)address); }

// ---------------------------------------------------------------- a big integer of bits, the simple way
typedef std::vector<uint8_t> Big;   // one bit per entry, least significant first
static Big big_of_limbs(const uint32_t *limb, int n) {
    Big b((size_t)(32 * n), 0);
    for (int i = 0; i < 32 * n; i++) b[(size_t)i] = (uint8_t)((limb[i >> 5] >> (i & 31)) & 1u);
    return b;
}
static int big_top(const Big &b) {
    for (int i = (int)b.size() - 1; i >= 0; i--)
        if (b[(size_t)i]) return i;
    return -1;
}
// schoolbook long division by a small number, a bit of the dividend at a time: q = n / d, the remainder is returned
static uint32_t big_divmod_small(const Big &n, uint32_t d, Big &q) {
    q.assign(n.size(), 0);
    uint64_t r = 0;
    for (int i = (int)n.size() - 1; i >= 0; i--) {
        r = 2 * r + n[(size_t)i];
        if (r >= d) r -= d, q[(size_t)i] = 1;
    }
    return (uint32_t)r;
}
// the bits of the float nearest, ties to even, to n * 2^-149 / count
static uint32_t big_mean(const Big &n, uint32_t count) {
    Big q;
    const uint32_t r = big_divmod_small(n, count, q);
    const int hb = big_top(q);
    uint32_t mant = 0;
    if (hb < 24) {   // every such integer is a float: its bits are the integer
        for (int i = hb; i >= 0; i--) mant = (mant << 1) | q[(size_t)i];
        if (2ull * r > count || (2ull * r == count && (mant & 1u))) mant++;
        return mant;
    }
    for (int i = hb; i > hb - 24; i--) mant = (mant << 1) | q[(size_t)i];
    bool sticky = r != 0;
    for (int i = hb - 25; i >= 0; i--) sticky |= q[(size_t)i] != 0;
    if (q[(size_t)(hb - 24)] && (sticky || (mant & 1u))) mant++;
    int s = hb - 23;
    if (mant >> 24) mant >>= 1, s++;
    return ((uint32_t)(s + 1) << 23) | (mant & 0x7FFFFFu);
}

// ---------------------------------------------------------------- totals as limbs: count * quotient + rest
constexpr int kN = statmc::kSumLimbs + 2;
struct Total { uint32_t limb[kN]; };
static Total total_of(uint64_t v, int shift, uint32_t times, uint32_t plus) {   // (v << shift) * times + plus
    Total t;
    memset(&t, 0, sizeof(t));
    for (int b = 0; b < 64; b++)
        if ((v >> b) & 1u) t.limb[(b + shift) >> 5] |= 1u << ((b + shift) & 31);
    uint64_t carry = plus;
    for (int i = 0; i < kN; i++) {
        const uint64_t x = (uint64_t)t.limb[i] * times + carry;
        t.limb[i] = (uint32_t)x, carry = x >> 32;
    }
    return t;
}

static int n_checked = 0;
static bool check(const char *what, const Total &t, uint32_t count) {
    const uint32_t got = statmc::tile_mean_bits(t.limb, kN, count), want = big_mean(big_of_limbs(t.limb, kN), count);
    n_checked++;
    if (got == want) return true;
    fprintf(stderr, "%s / %u: %08x, the long division gives %08x\n", what, count, got, want);
    return false;
}
static bool check_is(const char *what, const Total &t, uint32_t count, uint32_t bits) {
    const uint32_t got = statmc::tile_mean_bits(t.limb, kN, count);
    if (got != bits) fprintf(stderr, "%s / %u: %08x, expected %08x\n", what, count, got, bits);
    return check(what, t, count) && got == bits;
}

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;   // splitmix64, fixed seed
static uint64_t rng() {
    uint64_t z = (rng_state += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

static bool means() {
    bool ok = true;
    const uint32_t counts[5] = {1, 2, 3, 4095, 4096};
    for (uint32_t c : counts) {
        ok &= check_is("zero", total_of(0, 0, c, 0), c, 0u);
        // quotients on either side of 2^23 (the first normal float) and of 2^24 (the first that rounds), every kind of remainder
        const uint64_t around[8] = {(1u << 23) - 2, (1u << 23) - 1, 1u << 23, (1u << 23) + 1, (1u << 24) - 2, (1u << 24) - 1, 1u << 24, (1u << 24) + 1};
        for (uint64_t q : around) {
            const uint32_t rests[6] = {0, 1, c / 2 - (c > 2), c / 2, c / 2 + 1, c - 1};
            for (uint32_t r : rests)
                if (r < c) ok &= check("around 2^23 and 2^24", total_of(q, 0, c, r), c);
        }
        ok &= check_is("2^24 - 1 and all but nothing rounds up to 2^24", total_of((1u << 24) - 1, 0, c, c - 1), c, c == 1 ? 0x00FFFFFFu : 0x01000000u);
        // exact ties above 2^24: 2^24 + 1 goes down to even, 2^24 + 3 up to even; a remainder breaks the first upwards
        for (int shift = 0; shift < 230; shift += 13) {
            ok &= check_is("a tie, even below", total_of((1u << 24) + 1, shift, c, 0), c, (uint32_t)(shift + 2) << 23);
            ok &= check_is("a tie, odd below", total_of((1u << 24) + 3, shift, c, 0), c, ((uint32_t)(shift + 2) << 23) + 2);
            if (c > 1) ok &= check_is("a tie broken by the remainder", total_of((1u << 24) + 1, shift, c, 1 + (uint32_t)(rng() % (c - 1))), c, ((uint32_t)(shift + 2) << 23) + 1);
            if (shift && shift < 39) ok &= check("a tie broken far below", total_of((1ull << (24 + shift)) + (1ull << shift) + 1, 0, c, 0), c);
        }
        // exact ties below 2^24: the remainder is half the divisor
        if (c % 2 == 0) {
            ok &= check_is("half a unit, even below", total_of(6, 0, c, c / 2), c, 6u);
            ok &= check_is("half a unit, odd below", total_of(7, 0, c, c / 2), c, 8u);
            ok &= check_is("half a unit below one", total_of(0, 0, c, c / 2), c, 0u);
        }
        ok &= check_is("the largest finite float, every pixel", total_of(0xFFFFFF, 253, c, 0), c, 0x7F7FFFFFu);
        ok &= check_is("one", total_of(1, 149, c, 0), c, 0x3F800000u);
    }
    ok &= check_is("the smallest total: one unit over 4096 pixels", total_of(1, 0, 1, 0), 4096, 0u);
    ok &= check_is("one unit over two pixels ties to +0", total_of(1, 0, 1, 0), 2, 0u);
    ok &= check_is("three units over two pixels tie to two", total_of(3, 0, 1, 0), 2, 2u);
    ok &= check_is("2^-149 and the largest float over two pixels", total_of(0xFFFFFF, 253, 1, 1), 2, 0x7EFFFFFFu);   // (2^24 - 1) 2^252 and half a unit: a float and a little
    for (int it = 0; it < 1000; it++) {
        Total t;
        const int used = 1 + (int)(rng() % 8);   // below 2^256: the quotient is a finite float for every count
        for (int i = 0; i < kN; i++) {
            uint32_t w = i < used ? (uint32_t)rng() : 0u;
            if (it % 3 == 1) w >>= rng() % 32;
            if (it % 5 == 2 && (rng() & 1)) w = 0;
            if (it % 7 == 3) w = (rng() & 1) ? ~0u : 0u;
            t.limb[i] = w;
        }
        const uint32_t c = it % 4 == 0 ? counts[rng() % 5] : 1 + (uint32_t)(rng() % 4096);
        ok &= check("random totals", t, c);
    }
    return ok;
}

// ---------------------------------------------------------------- a whole film on the host
static void film_line(const char *name, int width, int height, int tile, uint32_t cap_bits, const std::vector<uint32_t> &px) {
    using namespace statmc;
    float cap;
    memcpy(&cap, &cap_bits, sizeof(cap));
    statmc_tile_scores out;
    memset(&out, 0, sizeof(out));
    out.mean = at<float>(1u << 20);
    TilesArgs a;
    fill_score_tiles_args(a, (uint16_t)width, (uint16_t)height, at<float>(16), tile, cap, &out);
    printf("%s : film %d %d", name, a.tiles_x, a.tiles_y);
    for (int ty = 0; ty < a.tiles_y; ty++)
        for (int tx = 0; tx < a.tiles_x; tx++) {
            uint64_t acc[kTileAccWords];
            memset(acc, 0, sizeof(acc));
            uint32_t n = 0, zero = 0, infinite = 0, clipped = 0, max_key = 0;
            for (int y = ty * tile; y < (ty + 1) * tile && y < height; y++)
                for (int x = tx * tile; x < (tx + 1) * tile && x < width; x++) {   // the kernel's pass, a pixel at a time
                    const uint32_t key = select_key(px[(size_t)y * (size_t)width + (size_t)x]);
                    n++, zero += key == 0, infinite += key == kSumInfinite, clipped += key > a.cap_key;
                    max_key = key > max_key ? key : max_key;
                    if (key == 0 || key > a.cap_key || key == kSumInfinite) continue;
                    const uint64_t M = sum_significand(key);
                    const int s = sum_shift(key), sh = (2 * s) & 31;
                    const uint64_t v = M << (s & 31), q = M * M, upper = q >> (32 - sh);
                    uint64_t *sum = &acc[s >> 5], *sq = &acc[kSumLimbs + ((2 * s) >> 5)];
                    sum[0] += (uint32_t)v, sum[1] += v >> 32;
                    sq[0] += (uint32_t)(q << sh), sq[1] += (uint32_t)upper, sq[2] += upper >> 32;
                }
            uint32_t limb[kTileLimbs];
            tile_capped_limbs(acc, kSumLimbs, false, a.cap_key, clipped, limb);
            const uint64_t sum_bits = sum_round_bits(limb, kSumLimbs + 2, kSumUnitExp);
            const uint32_t counted = n - (a.cap_key == kSumInfinite ? infinite : 0u);
            const uint32_t mean_bits = counted ? tile_mean_bits(limb, kSumLimbs + 2, counted) : 0u;
            tile_capped_limbs(acc + kSumLimbs, kSumSqLimbs, true, a.cap_key, clipped, limb);
            const uint64_t sq_bits = sum_round_bits(limb, kSumSqLimbs + 2, kSumSqUnitExp);
            printf(" %u %u %u %u %016" PRIx64 " %016" PRIx64 " %08x %08x", n, zero, infinite, clipped, sum_bits, sq_bits, mean_bits, max_key);
        }
    printf("\n");
}

int main(int argc, char **argv) {
    if (argc != 2) {
        fprintf(stderr, "usage: %s <table>\n", argv[0]);
        return 2;
    }
    if (!means()) return 1;
    FILE *f = fopen(argv[1], "r");
    if (!f) {
        perror(argv[1]);
        return 2;
    }
    printf("means : ok %d\n", n_checked);
    char word[64], name[128], why[512];
    int n_calls = 0;
    while (fscanf(f, "%63s", word) == 1) {
        why[0] = 0;
        if (strcmp(word, "tiles") == 0) {
            int width, height, tile, given;
            uint64_t score, p[8];
            uint32_t cap_bits;
            if (fscanf(f, "%127s %d %d %" SCNu64 " %d %" SCNu32 " %d", name, &width, &height, &score, &tile, &cap_bits, &given) != 7) {
                fprintf(stderr, "bad tiles line\n");
                return 2;
            }
            for (int i = 0; i < 8; i++)
                if (fscanf(f, "%" SCNu64, &p[i]) != 1) return 2;
            float cap;
            memcpy(&cap, &cap_bits, sizeof(cap));
            statmc_tile_scores out = {at<double>(p[0]), at<double>(p[1]), at<float>(p[2]), at<float>(p[3]),
                                      at<int32_t>(p[4]), at<int32_t>(p[5]), at<int32_t>(p[6]), at<int32_t>(p[7])};
            const statmc_tile_scores *op = given ? &out : nullptr;
            if (!statmc::check_score_tiles_call((uint16_t)width, (uint16_t)height, at<float>(score), tile, cap, op, statmc::SelectMsg{why, sizeof(why)})) {
                printf("%s : %s\n", name, why);
            } else {
                statmc::TilesArgs a;
                statmc::fill_score_tiles_args(a, (uint16_t)width, (uint16_t)height, at<float>(score), tile, cap, op);
                printf("%s : ok tiles %d %d %lld %08x %d\n", name, a.tiles_x, a.tiles_y, a.n_tiles, (unsigned)a.cap_key, a.vec);
            }
        } else if (strcmp(word, "film") == 0) {
            int width, height, tile;
            uint32_t cap_bits;
            if (fscanf(f, "%127s %d %d %d %" SCNu32, name, &width, &height, &tile, &cap_bits) != 5 || width < 1 || height < 1 || width * height > (1 << 20))
                return 2;
            std::vector<uint32_t> px((size_t)(width * height));
            for (size_t i = 0; i < px.size(); i++)
                if (fscanf(f, "%" SCNu32, &px[i]) != 1) return 2;
            film_line(name, width, height, tile, cap_bits, px);
        } else {
            fprintf(stderr, "bad table near '%s'\n", word);
            return 2;
        }
        n_calls++;
    }
    fclose(f);
    return n_calls > 0 ? 0 : 2;
}
