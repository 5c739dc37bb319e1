// Driver of tests/test_weight_layout_cpu.py: csrc/wlayout.h alone, plain g++.  Per input line "N K force nt {type row0 rows} x nt" prints
// "error <message>" or three lines: the scalars, the row-group types, the row-group offsets.
#include "../../qwen3-tts-rust_amd/csrc/wlayout.h"
#include <cstdio>
#include <iostream>

using namespace q3;

int main() {
    int N, K, force, nt;
    while (std::cin >> N >> K >> force >> nt) {
        std::vector<WTensor> t((size_t)nt);
        for (auto& x : t) std::cin >> x.type >> x.row0 >> x.rows;
        try {
            const WLayout L = plan_wlayout(t, N, K, force != 0);
            // Npad mapped qbytes | section offsets sc meta ty off total | section sizes qs sc meta ty off | nparts p0_type p0_off p1_rg0 p1_type p1_off p2_rg0 p2_type p2_off
            printf("%d %d %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %d %d %u %d %d %u %d %d %u\n", L.Npad, (int)L.mapped, L.qbytes, L.sc_at(), L.meta_at(),
                   L.ty_at(), L.off_at(), L.total(), L.qs_bytes, L.sc_bytes, L.meta_bytes, L.ty_bytes, L.off_bytes, L.nparts, L.p0_type, L.p0_off, L.p1_rg0,
                   L.p1_type, L.p1_off, L.p2_rg0, L.p2_type, L.p2_off);
            for (uint8_t v : L.rg_type) printf("%d ", v);
            printf("\n");
            for (uint32_t v : L.rg_off) printf("%u ", v);
            printf("\n");
        } catch (const std::exception& e) { printf("error %s\n", e.what()); }
    }
    return 0;
}
