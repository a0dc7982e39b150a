// CPU driver of csrc/attn_select.hpp for tests/test_attn_select.py: one case per stdin line -
//   name dims[40] has_bias has_mask has_lse drop_p ksplit has_parts part_rows big_gate persist_gate cus
// - through attn_parse and attn_select, one JSON line per case with every AttnLaunch field (an error: the status alone).
#include <stdio.h>
#include "../cobevt_amd/csrc/attn_select.hpp"

using namespace cobevt;

int main() {
    static const char* const kFamily[] = {"RESIDENT", "RESIDENT_BIG", "STREAM", "STREAM_DROP"};
    char name[128];
    while (scanf("%127s", name) == 1) {
        int dims[40], bias, mask, lse, ksplit, parts, big, persist, cus;
        float drop_p;
        long part_rows;
        for (int& d : dims) if (scanf("%d", &d) != 1) return 2;
        if (scanf("%d %d %d %f %d %d %ld %d %d %d", &bias, &mask, &lse, &drop_p, &ksplit, &parts, &part_rows, &big, &persist, &cus) != 10) return 2;
        AttnParams p;
        AttnHints h;
        AttnLaunch a = {};
        a.status = attn_parse(dims, bias != 0, mask != 0, lse != 0, drop_p, ksplit, parts != 0, part_rows, p, h);
        if (a.status == COBEVT_OK) a = attn_select(p, h, cus, AttnGates{big != 0, persist != 0});
        if (a.status != COBEVT_OK) { printf("{\"name\": \"%s\", \"status\": %d}\n", name, a.status); continue; }
        const auto b = [](bool v) { return v ? "true" : "false"; };
        printf("{\"name\": \"%s\", \"status\": %d, \"family\": \"%s\", \"NT\": %d, \"NW\": %d, \"MEAN\": %s, \"BIAS\": %s, \"MASK\": %s, "
               "\"RAGGED\": %s, \"W8\": %s, \"PERSIST\": %s, \"dtype\": %d, \"KT\": %d, \"grid\": [%u, %u, %u], \"block\": %d, \"lds\": %zu, "
               "\"qsplit\": %d, \"merge_grid\": %u}\n",
               name, a.status, kFamily[a.family], a.NT, a.NW, b(a.MEAN), b(a.BIAS), b(a.MASK), b(a.RAGGED), b(a.W8), b(a.PERSIST), a.dtype,
               a.KT, a.grid[0], a.grid[1], a.grid[2], a.block, a.lds, a.qsplit, a.merge_grid);
    }
    return 0;
}
