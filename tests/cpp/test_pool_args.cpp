// statmc_pool_args.h on its own: no library, no device, nothing but include/statmc.h.  Reads a table of calls -- the one
// tests/test_pool_cpu.py writes from its restatement of include/statmc.h -- and prints check_pool_call's verdict for each, and for
// the valid ones what fill_pool_args made of them.  The image "pointers" of the table are numbers: nothing is read through them.
//
//   call <name> <width> <height> <k> <n_entries> <entries given: 0 | 1> <entries listed>
//   entry <count_of>  <dst: channels max_moment n mean m2 m3 film_mean film_m2 mean_corr discriminator>  <src: the same ten>
//
// Output, one line per call:   <name> : ok wc hc vec {cnt_src cnt_dst moments film per entry}   or   <name> : <message>
#include <inttypes.h>
#include <stdio.h>
#include <string.h>

#include <vector>

#include "../../statmc_amd/csrc/statmc_pool_args.h"

static bool read_side(FILE *f, statmc_stat_type &t) {
    uint64_t p[8];
    int ch, mm;
    if (fscanf(f, "%d %d", &ch, &mm) != 2) return false;
    for (uint64_t &v : p)
        if (fscanf(f, "%" SCNu64, &v) != 1) return false;
    memset(&t, 0, sizeof(t));
    t.channels = ch;
    t.max_moment = mm;
    t.n = reinterpret_cast<int32_t *>((uintptr_t)p[0]);
    float **planes[7] = {&t.mean, &t.m2, &t.m3, &t.film_mean, &t.film_m2, &t.mean_corr, &t.discriminator};
    for (int i = 0; i < 7; i++) *planes[i] = reinterpret_cast<float *>((uintptr_t)p[1 + i]);
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
    char word[64], name[128];
    int n_calls = 0;
    while (fscanf(f, "%63s", word) == 1) {
        int width, height, k, n_entries, given, listed;
        if (strcmp(word, "call") != 0 || fscanf(f, "%127s %d %d %d %d %d %d", name, &width, &height, &k, &n_entries, &given, &listed) != 7) {
            fprintf(stderr, "bad table near '%s'\n", word);
            return 2;
        }
        std::vector<statmc_pool_entry> entries(listed);
        for (int i = 0; i < listed; i++) {
            int count_of;
            if (fscanf(f, "%63s %d", word, &count_of) != 2 || strcmp(word, "entry") != 0 || !read_side(f, entries[i].dst) ||
                !read_side(f, entries[i].src)) {
                fprintf(stderr, "bad entry %d of %s\n", i, name);
                return 2;
            }
            entries[i].count_of = count_of;
        }
        char why[512] = "";
        const statmc_pool_entry *arg = given ? entries.data() : nullptr;
        if (!statmc::check_pool_call((uint16_t)width, (uint16_t)height, k, arg, n_entries, statmc::PoolMsg{why, sizeof(why)})) {
            printf("%s : %s\n", name, why);
        } else {
            statmc::PoolArgs a;
            statmc::fill_pool_args(a, (uint16_t)width, (uint16_t)height, k, arg, n_entries);
            printf("%s : ok %d %d %d", name, a.wc, a.hc, a.vec);
            for (int i = 0; i < a.n_entries; i++)
                printf(" {%" PRIu64 " %" PRIu64 " %d %d}", (uint64_t)(uintptr_t)a.e[i].cnt_src, (uint64_t)(uintptr_t)a.e[i].cnt_dst, a.e[i].moments,
                       a.e[i].film);
            printf("\n");
        }
        n_calls++;
    }
    fclose(f);
    return n_calls > 0 ? 0 : 2;
}
