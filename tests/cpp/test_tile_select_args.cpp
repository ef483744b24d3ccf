// statmc_tile_select_args.h on its own: no library, no device, nothing but include/statmc.h.
//
// A table of lines -- the one tests/test_tile_select_cpu.py writes from its restatement of include/statmc.h:
//   select <name> <width> <height> <score> <tile> <q_den> <n_ranks> <q_num given: 0 / 1> <out given: 0 / 1> <q_num x 4> <value x 4> <n_below x 4> <n_equal x 4>
//   gate <name> <width> <height> <tile> <tile_value> <threshold as float bits> <closed> <open> <n_images> <src given> <dst given> <src x 4> <dst x 4> <result>
//   rank <name> <n> <q_num> <q_den>
//   film <name> <width> <height> <tile> <q_den> <n_ranks> <q_num x 4> <width * height pixels as float bits>
//   gatefilm <name> <width> <height> <tile> <threshold as float bits> <closed given: 0 / 1> <n_tiles tile values as float bits> [<n_tiles closed words>]
// The "pointers" of a select or gate line are numbers: nothing is read through them.  A film line is the whole select on the host
// (tile_select_host), a gatefilm line the gate's tile pass (gate_tiles_host).
// Output, one line per entry:   <name> : ok select <tiles_x> <tiles_y> <n_tiles> <vec>   |
//                               <name> : ok gate <tiles_x> <tiles_y> <n_tiles> <threshold key, 8 hex digits> <tile_shift> <vec>   |
//                               <name> : rank <rank>   |
//                               <name> : film <tiles_x> <tiles_y> then per tile, row-major, per rank <value bits, hex> <n_below> <n_equal>   |
//                               <name> : gatefilm <n_tiles> <n_open> <n_closed_now> <n_px_open> then per tile <open><closed>   |
//                               <name> : <message>
#include <inttypes.h>
#include <stdio.h>
#include <string.h>

#include <vector>

#include "../../statmc_amd/csrc/statmc_tile_select_args.h"

template <typename T>
static T *at(uint64_t address) { return reinterpret_cast<T *>((uintptr_t)address); }

static bool read_u64(FILE *f, uint64_t *v, int n) {
    for (int i = 0; i < n; i++)
        if (fscanf(f, "%" SCNu64, &v[i]) != 1) return false;
    return true;
}

int main(int argc, char **argv) {
    if (argc != 2) {
        fprintf(stderr, "usage: %s <table>\n", argv[0]);
        return 2;
    }
    FILE *f = fopen(argv[1], "r");
    if (!f) {
        perror(argv[1]);
        return 2;
    }
    char word[64], name[128], why[512];
    int n_calls = 0;
    while (fscanf(f, "%63s", word) == 1) {
        why[0] = 0;
        if (strcmp(word, "select") == 0) {
            int width, height, tile, q_den, n_ranks, q_given, out_given, q[4];
            uint64_t score, p[12];
            if (fscanf(f, "%127s %d %d %" SCNu64 " %d %d %d %d %d %d %d %d %d", name, &width, &height, &score, &tile, &q_den, &n_ranks, &q_given,
                       &out_given, &q[0], &q[1], &q[2], &q[3]) != 13 || !read_u64(f, p, 12))
                return 2;
            const int32_t q_num[4] = {q[0], q[1], q[2], q[3]};
            statmc_tile_quantiles out;
            for (int i = 0; i < 4; i++) out.value[i] = at<float>(p[i]), out.n_below[i] = at<int32_t>(p[4 + i]), out.n_equal[i] = at<int32_t>(p[8 + i]);
            const statmc_tile_quantiles *op = out_given ? &out : nullptr;
            const int32_t *qp = q_given ? q_num : nullptr;
            if (!statmc::check_tile_select_call((uint16_t)width, (uint16_t)height, at<float>(score), tile, qp, q_den, n_ranks, op,
                                                statmc::SelectMsg{why, sizeof(why)})) {
                printf("%s : %s\n", name, why);
            } else {
                statmc::TileSelectArgs a;
                statmc::fill_tile_select_args(a, (uint16_t)width, (uint16_t)height, at<float>(score), tile, qp, q_den, n_ranks, op);
                printf("%s : ok select %d %d %lld %d\n", name, a.tiles_x, a.tiles_y, a.n_tiles, a.vec);
            }
        } else if (strcmp(word, "gate") == 0) {
            int width, height, tile, n_images, src_given, dst_given;
            uint64_t tile_value, closed, open, s[4], d[4], result;
            uint32_t thr_bits;
            if (fscanf(f, "%127s %d %d %d %" SCNu64 " %" SCNu32 " %" SCNu64 " %" SCNu64 " %d %d %d", name, &width, &height, &tile, &tile_value, &thr_bits,
                       &closed, &open, &n_images, &src_given, &dst_given) != 11 || !read_u64(f, s, 4) || !read_u64(f, d, 4) || !read_u64(f, &result, 1))
                return 2;
            float thr;
            memcpy(&thr, &thr_bits, sizeof(thr));
            const void *src[4];
            void *dst[4];
            for (int i = 0; i < 4; i++) src[i] = at<void>(s[i]), dst[i] = at<void>(d[i]);
            if (!statmc::check_gate_call((uint16_t)width, (uint16_t)height, tile, at<float>(tile_value), thr, at<int32_t>(closed), at<int32_t>(open),
                                         src_given ? src : nullptr, dst_given ? dst : nullptr, n_images, at<statmc_gate_result>(result),
                                         statmc::SelectMsg{why, sizeof(why)})) {
                printf("%s : %s\n", name, why);
            } else {
                statmc::GateArgs a;
                statmc::fill_gate_args(a, (uint16_t)width, (uint16_t)height, tile, at<float>(tile_value), thr, at<int32_t>(closed), at<int32_t>(open),
                                       src, dst, n_images, at<statmc_gate_result>(result));
                printf("%s : ok gate %d %d %lld %08x %d %d\n", name, a.tiles_x, a.tiles_y, a.n_tiles, (unsigned)a.threshold_key, a.tile_shift, a.vec);
            }
        } else if (strcmp(word, "rank") == 0) {
            uint32_t n, num, den;
            if (fscanf(f, "%127s %" SCNu32 " %" SCNu32 " %" SCNu32, name, &n, &num, &den) != 4) return 2;
            printf("%s : rank %u\n", name, statmc::tile_select_rank(n, num, den));
        } else if (strcmp(word, "film") == 0) {
            int width, height, tile, q_den, n_ranks, q[4];
            if (fscanf(f, "%127s %d %d %d %d %d %d %d %d %d", name, &width, &height, &tile, &q_den, &n_ranks, &q[0], &q[1], &q[2], &q[3]) != 10 ||
                width < 1 || height < 1 || width * height > (1 << 20) || n_ranks < 1 || n_ranks > 4)
                return 2;
            std::vector<uint32_t> px((size_t)(width * height));
            for (size_t i = 0; i < px.size(); i++)
                if (fscanf(f, "%" SCNu32, &px[i]) != 1) return 2;
            const int32_t q_num[4] = {q[0], q[1], q[2], q[3]};
            statmc_tile_quantiles out;
            memset(&out, 0, sizeof(out));
            out.value[0] = at<float>(1u << 20);
            statmc::TileSelectArgs a;
            statmc::fill_tile_select_args(a, (uint16_t)width, (uint16_t)height, at<float>(16), tile, q_num, q_den, n_ranks, &out);
            const size_t n_tiles = (size_t)a.n_tiles;
            std::vector<float> value(4 * n_tiles);
            std::vector<int32_t> below(4 * n_tiles), equal(4 * n_tiles);
            std::vector<uint32_t> scratch((size_t)statmc::kTileMaxPixels);
            memset(&out, 0, sizeof(out));
            for (int i = 0; i < n_ranks; i++)
                out.value[i] = value.data() + (size_t)i * n_tiles, out.n_below[i] = below.data() + (size_t)i * n_tiles, out.n_equal[i] = equal.data() + (size_t)i * n_tiles;
            statmc::tile_select_host(a, px.data(), out, scratch.data());
            printf("%s : film %d %d", name, a.tiles_x, a.tiles_y);
            for (size_t t = 0; t < n_tiles; t++)
                for (int i = 0; i < n_ranks; i++) {
                    uint32_t v;
                    memcpy(&v, &value[(size_t)i * n_tiles + t], 4);
                    printf(" %08x %d %d", v, below[(size_t)i * n_tiles + t], equal[(size_t)i * n_tiles + t]);
                }
            printf("\n");
        } else if (strcmp(word, "gatefilm") == 0) {
            int width, height, tile, closed_given;
            uint32_t thr_bits;
            if (fscanf(f, "%127s %d %d %d %" SCNu32 " %d", name, &width, &height, &tile, &thr_bits, &closed_given) != 6 || width < 1 || height < 1) return 2;
            float thr;
            memcpy(&thr, &thr_bits, sizeof(thr));
            statmc::GateArgs a;
            statmc::fill_gate_args(a, (uint16_t)width, (uint16_t)height, tile, at<float>(16), thr, nullptr, at<int32_t>(32), nullptr, nullptr, 0, nullptr);
            const size_t n_tiles = (size_t)a.n_tiles;
            std::vector<uint32_t> values(n_tiles);
            std::vector<int32_t> closed(n_tiles), open(n_tiles);
            for (size_t t = 0; t < n_tiles; t++)
                if (fscanf(f, "%" SCNu32, &values[t]) != 1) return 2;
            for (size_t t = 0; closed_given && t < n_tiles; t++)
                if (fscanf(f, "%" SCNd32, &closed[t]) != 1) return 2;
            statmc_gate_result r;
            statmc::gate_tiles_host(a, values.data(), closed_given ? closed.data() : nullptr, open.data(), &r);
            printf("%s : gatefilm %lld %lld %lld %lld", name, (long long)r.n_tiles, (long long)r.n_open, (long long)r.n_closed_now, (long long)r.n_px_open);
            for (size_t t = 0; t < n_tiles; t++) printf(" %d/%d", open[t], closed_given ? closed[t] : -1);
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
