// One line of tests/golden/rows_select/cases.txt, read from stdin by tests/rows_select_main.cpp (the header under test) and by
// tools/rows_select_oracle.cpp (a source tree's real entry points):
//   name entry nd dims[nd] nf flags[nf] rc64_prefetch ln_linear64 ln64_blocks
// entry: chain | proj | small_k | bev | mean.  flags[0] = the required pointers: 1 all given, 0 the first one null, 2 dims null;
// flags[1 ..] = the nullable pointers whose null-ness the entry point looks at, in argument order:
//   chain  skip post_gamma post_beta wnext out_next      proj  pre_scale pre_shift skip      small_k  residual pre_scale pre_shift
#pragma once
#include <stdio.h>
#include <string.h>

struct RowsCase {
    char name[128], entry[16];
    int nd, nf;
    long dims[16];
    int idims[16];            // the same as int, for the two int32 entry points
    int flag[8];
    int gates[3];
    bool is(const char* e) const { return strcmp(entry, e) == 0; }
};

// 1 = a case was read, 0 = end of input, -1 = malformed
inline int read_rows_case(RowsCase& c) {
    if (scanf("%127s", c.name) != 1) return 0;
    if (scanf("%15s %d", c.entry, &c.nd) != 2 || c.nd < 0 || c.nd > 16) return -1;
    for (int i = 0; i < c.nd; ++i) {
        if (scanf("%ld", &c.dims[i]) != 1) return -1;
        c.idims[i] = (int)c.dims[i];
    }
    if (scanf("%d", &c.nf) != 1 || c.nf < 1 || c.nf > 8) return -1;
    for (int i = 0; i < 8; ++i) c.flag[i] = 0;
    for (int i = 0; i < c.nf; ++i) if (scanf("%d", &c.flag[i]) != 1) return -1;
    if (scanf("%d %d %d", &c.gates[0], &c.gates[1], &c.gates[2]) != 3) return -1;
    return 1;
}
