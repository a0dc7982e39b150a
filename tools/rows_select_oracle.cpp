// The five row-local entry points of a source tree as a CPU program (tools/rows_select_fixture.py links it with the tree's kernel
// files, all compiled with attn_select_shim.hpp force-included): reads the case lines of tests/golden/rows_select/cases.txt on stdin,
// calls the real entry point with placeholder pointers and prints "case <name>", the shim's launch records and "rc <code>".  The
// environment gates are read by the tree's own code, so a case's gate columns are not used here: run one process per gate setting.
#include "../include/cobevt_hip.h"
#include "rows_select_case.hpp"

int main() {
    static char ptr[16];
    const float* const fp = (const float*)ptr;
    RowsCase c;
    int got;
    while ((got = read_rows_case(c)) == 1) {
        const auto opt = [&](int i) { return c.flag[i] ? ptr : nullptr; };
        const auto optf = [&](int i) { return c.flag[i] ? fp : nullptr; };
        const void* first = c.flag[0] == 0 ? nullptr : ptr;
        const bool nd = c.flag[0] == 2;
        int rc = -100;
        printf("case %s\n", c.name);
        if (c.is("chain"))
            rc = cobevt_attn_mlp_chain(first, opt(1), ptr, ptr, fp, ptr, fp, ptr, fp, optf(2), optf(3), opt(4), fp, opt(5), nd ? nullptr : c.idims,
                                       1e-5f, 1e-5f, 1e-5f, nullptr);
        else if (c.is("proj"))
            rc = cobevt_proj_chain(first, optf(1), optf(2), opt(3), ptr, fp, ptr, ptr, fp, ptr, nd ? nullptr : c.idims, 1e-5f, nullptr);
        else if (c.is("small_k"))
            rc = cobevt_linear_rows_small_k(first, ptr, fp, opt(1), optf(2), optf(3), ptr, nd ? nullptr : c.dims, 1e-5f, nullptr);
        else if (c.is("bev"))
            rc = cobevt_bev_embed_linear_rows_small_k((const float*)first, fp, fp, fp, fp, ptr, ptr, fp, ptr, nd ? nullptr : c.dims, 1e-5f, nullptr);
        else if (c.is("mean"))
            rc = cobevt_mean_linear_rows_small_k(first, ptr, fp, ptr, nd ? nullptr : c.dims, 1e-5f, nullptr);
        printf("rc %d\n", rc);
    }
    return got == 0 ? 0 : 2;
}
