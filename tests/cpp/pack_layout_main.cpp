// pack_layout_main.cpp -- prints the segment-table layout of a packed context (vit.cpp_amd/csrc/packed_context.h PackLayout) as JSON: for cap in
// {1, 3, 16} and each of the 16 subsets of the parts (bit 0 dense, 1 depth, 2 u8, 3 rollout) every accessor and ints().  No device call; the test
// (tests/test_cpu_pack_layout.py) compares the output with tests/golden/pack_layout.json, which the same program printed from the layout as it was
// written by hand, one conditional offset per part.
#include <cstdio>

#include "csrc/packed_context.h"

int main() {
    const size_t caps[3] = {1, 3, 16};
    printf("[");
    for (int c = 0; c < 3; ++c)
        for (unsigned parts = 0; parts < 16; ++parts) {
            const PackLayout at{caps[c], parts};
            printf("%s\n {\"cap\": %zu, \"parts\": %u, \"row0\": %zu, \"qb0\": %zu, \"toff\": %zu, \"tile0\": %zu, \"seg\": %zu, \"ftile0\": %zu, \"otile0\": %zu, "
                   "\"dseg\": %zu, \"ptile0\": %zu, \"pseg\": %zu, \"rblk0\": %zu, \"sq0\": %zu, \"ints\": %zu}",
                   c || parts ? "," : "", caps[c], parts, at.row0(), at.qb0(), at.toff(), at.tile0(), at.seg(), at.ftile0(), at.otile0(), at.dseg(), at.ptile0(), at.pseg(),
                   at.rblk0(), at.sq0(), at.ints());
        }
    printf("\n]\n");
    return 0;
}
