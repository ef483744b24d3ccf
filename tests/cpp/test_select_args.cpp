// statmc_select_args.h on its own: no library, no device, nothing but include/statmc.h.  Reads a table of calls -- the one
// tests/test_score_select_cpu.py writes from its restatement of include/statmc.h -- and prints check_select_call's /
// check_count_above_call's verdict for each, and for the valid ones what fill_select_args / fill_count_above_args made of them.  The
// image "pointers" of the table are numbers: nothing is read through them.  ranks and thresholds are host arrays and are real.
//
//   select <name> <width> <height>  <score result workspace> <workspace_bytes>  <ranks given: 0 / 1> <n_ranks> <k> <k ranks>
//   count <name> <width> <height>  <score counts>  <thresholds given: 0 / 1> <n_thresholds> <k> <k thresholds as float bits>
//   key <name> <float bits>
//
// Output, one line per call:   <name> : ok select <workspace bytes> <chunks> <grid> <vec> <ranks ...>   |
//                              <name> : ok count <chunks> <grid> <vec> <keys as 8 hex digits ...>   |   <name> : key <8 hex digits>   |
//                              <name> : <message>
#include <inttypes.h>
#include <stdio.h>
#include <string.h>

#include <vector>

#include "../../statmc_amd/csrc/statmc_select_args.h"

template <typename T>
static T *at(uint64_t address) { return reinterpret_cast<T *>((uintptr_t)address); }

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
    if (statmc::select_workspace_bytes() != statmc::select_workspace_bytes() || statmc::select_workspace_bytes() % 8 != 0) {
        fprintf(stderr, "the workspace helper is not a pure multiple of 8\n");
        return 2;
    }
    char word[64], name[128], why[512];
    int n_calls = 0;
    while (fscanf(f, "%63s", word) == 1) {
        int width, height, given, n, k;
        why[0] = 0;
        if (strcmp(word, "select") == 0) {
            uint64_t p[3], ws_bytes;
            if (fscanf(f, "%127s %d %d %" SCNu64 " %" SCNu64 " %" SCNu64 " %" SCNu64 " %d %d %d", name, &width, &height, &p[0], &p[1], &p[2], &ws_bytes,
                       &given, &n, &k) != 10 || k < 0 || k > 64) {
                fprintf(stderr, "bad select line\n");
                return 2;
            }
            std::vector<int64_t> ranks((size_t)k);
            for (int i = 0; i < k; i++)
                if (fscanf(f, "%" SCNd64, &ranks[(size_t)i]) != 1) return 2;
            const int64_t *rp = given ? ranks.data() : nullptr;
            if (!statmc::check_select_call((uint16_t)width, (uint16_t)height, at<float>(p[0]), rp, n, at<statmc_select_result>(p[1]), at<void>(p[2]),
                                           (size_t)ws_bytes, statmc::SelectMsg{why, sizeof(why)})) {
                printf("%s : %s\n", name, why);
            } else {
                statmc::SelectArgs a;
                statmc::fill_select_args(a, (uint16_t)width, (uint16_t)height, at<float>(p[0]), rp, n, at<statmc_select_result>(p[1]), at<void>(p[2]));
                printf("%s : ok select %zu %lld %d %d", name, statmc::select_workspace_bytes(), a.n_chunks, a.grid, a.vec);
                for (int i = 0; i < a.n_ranks; i++) printf(" %lld", a.rank[i]);
                printf("\n");
            }
        } else if (strcmp(word, "count") == 0) {
            uint64_t p[2];
            if (fscanf(f, "%127s %d %d %" SCNu64 " %" SCNu64 " %d %d %d", name, &width, &height, &p[0], &p[1], &given, &n, &k) != 8 || k < 0 || k > 64) {
                fprintf(stderr, "bad count line\n");
                return 2;
            }
            std::vector<float> thresholds((size_t)k);
            for (int i = 0; i < k; i++) {
                uint32_t b;
                if (fscanf(f, "%" SCNu32, &b) != 1) return 2;
                memcpy(&thresholds[(size_t)i], &b, sizeof(b));
            }
            const float *tp = given ? thresholds.data() : nullptr;
            if (!statmc::check_count_above_call((uint16_t)width, (uint16_t)height, at<float>(p[0]), tp, n, at<int64_t>(p[1]),
                                                statmc::SelectMsg{why, sizeof(why)})) {
                printf("%s : %s\n", name, why);
            } else {
                statmc::CountAboveArgs a;
                statmc::fill_count_above_args(a, (uint16_t)width, (uint16_t)height, at<float>(p[0]), tp, n, at<int64_t>(p[1]));
                printf("%s : ok count %lld %d %d", name, a.n_chunks, a.grid, a.vec);
                for (int i = 0; i < a.n_thresholds; i++) printf(" %08x", (unsigned)a.key[i]);
                printf("\n");
            }
        } else if (strcmp(word, "key") == 0) {
            uint32_t b;
            if (fscanf(f, "%127s %" SCNu32, name, &b) != 2) return 2;
            printf("%s : key %08x\n", name, (unsigned)statmc::select_key(b));
        } else {
            fprintf(stderr, "bad table near '%s'\n", word);
            return 2;
        }
        n_calls++;
    }
    fclose(f);
    return n_calls > 0 ? 0 : 2;
}
