// The attention entry point of a source tree as a CPU program (tools/attn_select_fixture.py builds it with attn_select_shim.hpp
// force-included): reads the case lines of tests/golden/attn_select/cases.txt on stdin, calls window_attention_impl with
// placeholder pointers and prints "case <name>", the shim's launch records and "rc <code>".  The two environment gates are read
// by the tree's own code, so a case's gate columns are not used here: run one process per gate setting.
#include "attention.hip"
#include "attention_resident.hip"

int main() {
    char name[128];
    static char ptr[16];
    while (scanf("%127s", name) == 1) {
        int dims[40], bias, mask, lse, ksplit, parts, big, persist, cus;
        float drop_p;
        long part_rows;
        for (int& d : dims) if (scanf("%d", &d) != 1) return 2;
        if (scanf("%d %d %d %f %d %d %ld %d %d %d", &bias, &mask, &lse, &drop_p, &ksplit, &parts, &part_rows, &big, &persist, &cus) != 10) return 2;
        printf("case %s\n", name);
        const int rc = window_attention_impl(ptr, ptr, ptr, ptr, lse ? (float*)ptr : nullptr, bias ? (const float*)ptr : nullptr,
                                             mask ? (const float*)ptr : nullptr, dims, 1.f, drop_p, 0u, nullptr, nullptr, ksplit,
                                             parts ? ptr : nullptr, parts ? (float*)ptr : nullptr, part_rows);
        printf("rc %d\n", rc);
    }
    return 0;
}
