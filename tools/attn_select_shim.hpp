// Force-included in front of csrc/attention.hip + csrc/attention_resident.hip when tools/attn_select_fixture.py compiles them
// for the HOST only: every kernel launch becomes a printed record (demangled instantiation, grid, block, LDS, the resident
// kernels' qsplit argument) instead of a launch, so the real entry point tells which kernel it would run.  No GPU involved.
#pragma once
#include <hip/hip_runtime.h>
#include <cxxabi.h>
#include <stdio.h>
#include <stdlib.h>
#include <tuple>
#include <typeinfo>

namespace attn_oracle {

template <auto K> struct Tag {};

inline int last_int(int v) { return v; }                   // (AttnParams, int qsplit): the resident kernels
template <class T> int last_int(const T&) { return 0; }

template <auto K, class... A> void record(dim3 grid, dim3 block, size_t lds, A... args) {
    char* name = abi::__cxa_demangle(typeid(Tag<K>).name(), nullptr, nullptr, nullptr);
    const int qsplit = last_int(std::get<sizeof...(A) - 1>(std::tuple<A...>(args...)));
    printf("launch %s | %u %u %u %u %zu %d\n", name, grid.x, grid.y, grid.z, block.x, lds, qsplit);
    free(name);
}

}  // namespace attn_oracle

#undef hipLaunchKernelGGL
#define hipLaunchKernelGGL(kernel, grid, block, lds, stream, ...) attn_oracle::record<kernel>(grid, block, lds, __VA_ARGS__)
#define hipGetLastError() hipSuccess
