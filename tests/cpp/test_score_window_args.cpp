// statmc_score_window_args.h on its own: no library, no device, nothing but include/statmc.h behind it.  Reads a table of calls --
// the one tests/test_score_window_cpu.py writes from its restatement of include/statmc.h -- and prints check_score_window_call's
// verdict for each, and for the valid ones what fill_score_window_args made of them.  The image "pointers" of the table are
// numbers: nothing is read through them.
//
//   window <name> <width> <height>  <score out>  <op> <radius>
//
// Output, one line per call:   <name> : ok window <tiles x> <tiles y> <lds bytes> <vec in> <vec out> <identity as 8 hex digits>   |
//                              <name> : <message>
#include <inttypes.h>
#include <stdio.h>
#include <string.h>

#include "../../statmc_amd/csrc/statmc_score_window_args.h"

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
    char word[64], name[128], why[512];
    int n_calls = 0;
    while (fscanf(f, "%63s", word) == 1) {
        int width, height, op, radius;
        uint64_t p[2];
        why[0] = 0;
        if (strcmp(word, "window") != 0) {
            fprintf(stderr, "bad table near '%s'\n", word);
            return 2;
        }
        if (fscanf(f, "%127s %d %d %" SCNu64 " %" SCNu64 " %d %d", name, &width, &height, &p[0], &p[1], &op, &radius) != 7) {
            fprintf(stderr, "bad window line\n");
            return 2;
        }
        if (!statmc::check_score_window_call((uint16_t)width, (uint16_t)height, at<float>(p[0]), op, radius, at<float>(p[1]),
                                             statmc::SelectMsg{why, sizeof(why)})) {
            printf("%s : %s\n", name, why);
        } else {
            statmc::ScoreWindowArgs a;
            statmc::fill_score_window_args(a, (uint16_t)width, (uint16_t)height, at<float>(p[0]), op, radius, at<float>(p[1]));
            if (a.score != at<float>(p[0]) || a.out != at<float>(p[1]) || a.width != width || a.height != height || a.op != op || a.radius != radius) {
                fprintf(stderr, "%s: the argument block does not hold the call\n", name);
                return 2;
            }
            printf("%s : ok window %u %u %u %d %d %08x\n", name, a.tiles_x, a.tiles_y, a.lds_bytes, a.vec_in, a.vec_out,
                   (unsigned)statmc::window_identity(a.op));
        }
        n_calls++;
    }
    fclose(f);
    return n_calls > 0 ? 0 : 2;
}
