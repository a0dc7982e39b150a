// CPU driver of csrc/rows_select.hpp for tests/test_rows_select.py: one case per stdin line (rows_select_case.hpp) through the entry
// point's parse and select functions, one JSON line per case: status, kernel instantiation, grid, block, LDS bytes, nblk (an error:
// the status alone).
#include "../cobevt_amd/csrc/rows_select.hpp"
#include "rows_select_case.hpp"

using namespace cobevt;

static void kernel_name(const RowsLaunch& l, char* out, size_t n) {
    const auto b = [](bool v) { return v ? "true" : "false"; };
    switch (l.family) {
        case ROWS_CHAIN: snprintf(out, n, "row_chain_kernel<%d, %d, %s, %s>", l.NPASS, l.ROWS, b(l.FULL), b(l.MLP)); break;
        case ROWS_CHAIN64: snprintf(out, n, "row_chain64_kernel<%d, %d, %s>", l.NNT, l.NW, b(l.PF)); break;
        case ROWS_CHAIN_F32: snprintf(out, n, "row_chain_f32_kernel"); break;
        case ROWS_PROJ128: snprintf(out, n, "proj_chain128_kernel<%d, %d>", l.NNT, l.NW); break;
        case ROWS_LN_LINEAR64: snprintf(out, n, "ln_linear64_kernel<%d, %d>", l.NNT, l.NW); break;
        case ROWS_GEMM3: snprintf(out, n, "gemm_rows3_kernel<%s, %d>", b(l.EMB), l.ROWS); break;
        case ROWS_GEMM3_F32: snprintf(out, n, "gemm_rows3_f32_kernel"); break;
        case ROWS_BEV_QUERY: snprintf(out, n, "bev_query_kernel<%d>", l.NW); break;
    }
}

int main() {
    RowsCase c;
    int got;
    while ((got = read_rows_case(c)) == 1) {
        const RowsGates gates = {c.gates[0], c.gates[1] != 0, c.gates[2]};
        const bool req = c.flag[0] != 0, nd = c.flag[0] == 2;
        const auto f = [&](int i) { return c.flag[i] != 0; };
        RowsLaunch l = {};
        if (c.is("chain") || c.is("proj")) {
            ChainShape s;
            const bool chain = c.is("chain");
            l.status = chain ? chain_parse(nd ? nullptr : c.idims, req, f(1), f(2), f(3), f(4), f(5), s)
                             : proj_parse(nd ? nullptr : c.idims, req, f(1), f(2), f(3), s);
            if (l.status == COBEVT_OK) l = chain ? chain_select(s, gates) : proj_select(s);
        } else {
            RowsGemmShape s;
            const long* dims = nd ? nullptr : c.dims;
            if (c.is("small_k")) {
                l.status = small_k_parse(dims, req, f(1), f(2), f(3), s);
                if (l.status == COBEVT_OK) l = small_k_select(s, gates);
            } else if (c.is("bev")) {
                l.status = bev_embed_parse(dims, req, s);
                if (l.status == COBEVT_OK) l = bev_embed_select(s);
            } else if (c.is("mean")) {
                l.status = mean_parse(dims, req, s);
                if (l.status == COBEVT_OK) l = mean_select(s);
            } else {
                return 2;
            }
        }
        if (l.status != COBEVT_OK) { printf("{\"name\": \"%s\", \"status\": %d}\n", c.name, l.status); continue; }
        char kernel[96];
        kernel_name(l, kernel, sizeof kernel);
        printf("{\"name\": \"%s\", \"status\": 0, \"kernel\": \"%s\", \"grid\": [%u, 1, 1], \"block\": %d, \"lds\": %zu, \"nblk\": %d}\n", c.name, kernel,
               l.grid, l.block, l.lds, l.nblk);
    }
    return got == 0 ? 0 : 2;
}
