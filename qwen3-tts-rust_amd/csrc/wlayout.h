// wlayout.h -- the packed layout of one quantised weight matrix (Q8Mat, kernels.h) as a host-only rule: no HIP, plain g++
// (tests/test_weight_layout_cpu.py).  build_q8mat (transformer.cpp) is its only consumer: the engine and the parity ops build from the same plan.
#pragma once
#include <cstddef>
#include <cstdint>
#include <stdexcept>
#include <vector>

namespace q3 {

// bytes of one 32-row group of K columns in HBM, by ggml type (8 = Q8_0, 13 = Q5_K, 14 = Q6_K)
inline size_t q3_rowgroup_bytes(int type, int K) { return type == 13 ? (size_t)(K / 256) * 5120 : type == 14 ? (size_t)(K / 256) * 6144 : (size_t)(K / 32) * 1024; }
// bytes of one GGUF row of K columns: Q8_0 blocks of 34, Q5_K / Q6_K super-blocks of 176 / 210
inline size_t q3_gguf_row_bytes(int type, int K) { return type == 13 ? (size_t)(K / 256) * 176 : type == 14 ? (size_t)(K / 256) * 210 : (size_t)(K / 32) * 34; }

struct WTensor { int type, row0, rows; }; // ggml type, first row in the fused matrix, row count

// One device blob [quants | scales | meta | types | offsets].  Uniform (every tensor Q8_0, any N, rows zero-padded to 32): 1-KiB tiles, no meta,
// no offsets, no tensor map.  Mapped (a K-quant tensor, or force_map): every 32-row group has a type and a 16-byte-unit offset, tensors start and
// end on row groups, and runs of equal type -- at most 3 -- are the tensor map the kernels read from their arguments.  Row groups no tensor covers
// stay Q8_0-typed zero tiles.
struct WLayout {
    int N = 0, Npad = 0, K = 0;
    bool mapped = false;
    std::vector<WTensor> tensors;
    std::vector<uint8_t> rg_type; std::vector<uint32_t> rg_off;    // [Npad / 32]
    size_t qs_bytes = 0, sc_bytes = 0, meta_bytes = 0, ty_bytes = 0, off_bytes = 0; // sections, in blob order; types and offsets rounded up to 16
    size_t qbytes = 0;                                              // Q8Mat::qbytes: qs_bytes when mapped, else 0 (= Npad * K)
    int nparts = 0, p1_rg0 = 0x7fffffff, p2_rg0 = 0x7fffffff, p0_type = 0, p1_type = 0, p2_type = 0; uint32_t p0_off = 0, p1_off = 0, p2_off = 0;
    size_t sc_at() const { return qs_bytes; }
    size_t meta_at() const { return sc_at() + sc_bytes; }
    size_t ty_at() const { return meta_at() + meta_bytes; }
    size_t off_at() const { return ty_at() + ty_bytes; }
    size_t total() const { return off_at() + off_bytes; }
};

inline WLayout plan_wlayout(const std::vector<WTensor>& tensors, int N, int K, bool force_map) {
    auto need = [](bool ok, const char* msg) { if (!ok) throw std::runtime_error(msg); };
    need(K > 0 && K % 256 == 0, "K must be a multiple of 256");
    need(N > 0 && !tensors.empty(), "bad matrix shape");
    WLayout L;
    L.N = N; L.Npad = (N + 31) & ~31; L.K = K; L.tensors = tensors; L.mapped = force_map;
    for (const WTensor& t : tensors) {
        need(t.type == 8 || t.type == 13 || t.type == 14, "unsupported weight type (Q8_0, Q5_K, Q6_K)");
        L.mapped = L.mapped || t.type != 8;
    }
    const int nrg = L.Npad / 32;
    L.rg_type.assign((size_t)nrg, 8);
    for (const WTensor& t : tensors) {
        need(t.rows > 0 && t.row0 >= 0 && t.row0 + t.rows <= L.Npad, "bad row range");
        if (!L.mapped) continue;
        need(t.rows % 32 == 0 && t.row0 % 32 == 0, "tensor rows must be a multiple of 32");
        for (int i = 0; i < t.rows / 32; i++) L.rg_type[(size_t)(t.row0 / 32 + i)] = (uint8_t)t.type;
    }
    L.rg_off.resize((size_t)nrg);
    for (int i = 0; i < nrg; i++) { L.rg_off[(size_t)i] = (uint32_t)(L.qs_bytes / 16); L.qs_bytes += q3_rowgroup_bytes(L.rg_type[(size_t)i], K); }
    need(L.qs_bytes / 16 < (1ull << 32), "matrix too large for 32-bit row-group offsets");
    L.sc_bytes = (size_t)L.Npad * (K / 32) * 2;
    L.ty_bytes = (size_t)((nrg + 15) & ~15);
    if (!L.mapped) return L;
    L.meta_bytes = (size_t)L.Npad * (K / 256) * 16; L.off_bytes = (size_t)((nrg * 4 + 15) & ~15); L.qbytes = L.qs_bytes;
    int last = -1;
    for (int i = 0; i < nrg; i++) {
        if (last == L.rg_type[(size_t)i]) continue;
        last = L.rg_type[(size_t)i];
        need(L.nparts < 3, "more than 3 runs of weight types in one fused matrix");
        if (L.nparts == 0) { L.p0_type = last; L.p0_off = L.rg_off[(size_t)i]; }
        else if (L.nparts == 1) { L.p1_rg0 = i; L.p1_type = last; L.p1_off = L.rg_off[(size_t)i]; }
        else { L.p2_rg0 = i; L.p2_type = last; L.p2_off = L.rg_off[(size_t)i]; }
        L.nparts++;
    }
    return L;
}

} // namespace q3
