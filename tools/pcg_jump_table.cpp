// pcg_jump_table.cpp -- stand-alone driver of csrc/dzo_pcg.h (no GPU, no HIP): the jump ahead of the PCG32 stream that the
// basin-hopping kernels use, against advancing one draw at a time.  tests/test_basin_twin.py compares every line with the
// Python twin.
//
//   pcg_jump_table STATE K [K ...]      STATE in hex, every K in decimal
//   one line per K (hex):   K  pcg_jump(STATE, K)  STATE advanced K times  extract(of that state)  map.a  map.c
//
//   g++ -std=c++17 -Wall -Werror -fsanitize=address,undefined tools/pcg_jump_table.cpp -o pcg_jump_table
#include <cstdio>
#include <cstdlib>

#include "../dzoptimization.jl_amd/csrc/dzo_pcg.h"

using namespace dzo;

int main(int argc, char **argv) {
    if (argc < 3) { fprintf(stderr, "usage: pcg_jump_table STATE K [K ...]\n"); return 1; }
    const uint64_t state = strtoull(argv[1], nullptr, 16);
    for (int i = 2; i < argc; ++i) {
        const uint64_t k = strtoull(argv[i], nullptr, 10);
        if (k > (1u << 24)) { fprintf(stderr, "K = %s is too many single advances\n", argv[i]); return 2; }
        uint64_t s = state;
        for (uint64_t j = 0; j < k; ++j) (void)pcg_draw(s);
        const PcgMap map = pcg_jump_map(k);
        printf("%llx %llx %llx %x %llx %llx\n", (unsigned long long)k, (unsigned long long)pcg_jump(state, k), (unsigned long long)s,
               (unsigned)pcg_extract(s), (unsigned long long)map.a, (unsigned long long)map.c);
    }
    return 0;
}
