// Driver of tests/test_onnx_shape_cpu.py: the host-only rules of the ONNX executor (csrc/onnx_shape.h) against plain restatements over small
// grids, alone, plain g++ under the host sanitizers.  It checks everything itself, prints one "family checked" line per family and exits 1 at
// the first disagreement.
#include "../../qwen3-tts-rust_amd/csrc/onnx_shape.h"
#include <cstdio>
#include <cstdlib>

using namespace q3::xs;

#define REQUIRE(cond) do { if (!(cond)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); std::exit(1); } } while (0)
template <typename F> static bool refuses(F&& f) { try { f(); } catch (const ShapeError&) { return true; } return false; }

// every axis in [-rank - 3, rank + 3] for ranks 0..4: accepted exactly inside [-rank, rank) (and at rank itself where the end is allowed)
static long check_axes() {
    long n = 0;
    for (int64_t rank = 0; rank <= 4; rank++) for (int end_ok = 0; end_ok < 2; end_ok++) for (int64_t a = -rank - 3; a <= rank + 3; a++, n++) {
        const bool ok = a >= -rank && (a < rank || (end_ok && a == rank));
        if (!ok) { REQUIRE(refuses([&] { axis_of(a, rank, "Op", end_ok != 0); })); continue; }
        const int64_t got = axis_of(a, rank, "Op", end_ok != 0);
        REQUIRE(got == (a < 0 ? a + rank : a) && got >= 0 && got <= rank);
    }
    REQUIRE(refuses([] { norm_axes({0, 2}, 2); }) && norm_axes({-1, 0, 1, -2}, 2) == Shape({0, 1}));
    try { axis_of(5, 2, "Softmax"); REQUIRE(false); } catch (const ShapeError& e) { REQUIRE(std::string(e.what()).rfind("Softmax: axis out of range", 0) == 0); }
    return n;
}

// Slice against an index-by-index walk: the adjusted start and end clamped as the operator's text says (positive step: both into [0, dim];
// negative step: start into [0, dim - 1], end into [-1, dim - 1]), then one index at a time; every index taken must exist
static long check_slice() {
    long n = 0;
    for (int64_t dim = 0; dim <= 5; dim++) for (int64_t start = -dim - 2; start <= dim + 2; start++) for (int64_t end = -dim - 2; end <= dim + 2; end++)
        for (int64_t step : {-3, -2, -1, 1, 2, 3}) {
            std::vector<int64_t> want;
            int64_t s = start < 0 ? start + dim : start, e = end < 0 ? end + dim : end;
            if (dim > 0) {
                auto clamp = [](int64_t v, int64_t lo, int64_t hi) { return v < lo ? lo : v > hi ? hi : v; };
                if (step > 0) { s = clamp(s, 0, dim); e = clamp(e, 0, dim); for (int64_t i = s; i < e; i += step) want.push_back(i); }
                else { s = clamp(s, 0, dim - 1); e = clamp(e, -1, dim - 1); for (int64_t i = s; i > e; i += step) want.push_back(i); }
            }
            const SliceAxis g = slice_axis(dim, start, end, step);
            REQUIRE(g.count == (int64_t)want.size() && g.step == step);
            for (int64_t k = 0; k < g.count; k++) { const int64_t i = g.start + k * g.step; REQUIRE(i == want[(size_t)k] && i >= 0 && i < dim); }
            n++;
        }
    REQUIRE(refuses([] { slice_axis(4, 0, 4, 0); }));
    // the extreme bounds exporters write for "to the end" / "to the beginning"
    const int64_t big = std::numeric_limits<int64_t>::max(), small = std::numeric_limits<int64_t>::min() + 1;
    REQUIRE(slice_axis(5, 2, big, 1).count == 3 && slice_axis(5, 3, small, -1).count == 4 && slice_axis(5, big, small, -2).count == 3);
    return n;
}

// Conv output sizes against a count of the window positions that fit into the padded row; ConvTranspose against the extent its taps reach
static long check_conv() {
    long n = 0;
    const char* modes[] = {"NOTSET", "VALID", "SAME_UPPER", "SAME_LOWER"};
    for (int64_t in = 1; in <= 9; in++) for (int64_t k = 1; k <= 4; k++) for (int64_t s = 1; s <= 3; s++) for (int64_t d = 1; d <= 3; d++) {
        const int64_t eff = (k - 1) * d + 1;
        auto fits = [&](int64_t padded) { int64_t c = 0; for (int64_t o = 0; o * s + eff <= padded; o++) c++; return c; };
        for (const char* m : modes) for (int64_t pb = 0; pb <= 2; pb++) for (int64_t pe = 0; pe <= 2; pe++) {
            const std::string mode = m;
            if (mode != "NOTSET" && (pb || pe)) continue;   // explicit pads go with NOTSET
            const ConvDim g = conv_dim(in, k, s, d, pb, pe, mode);
            if (mode == "NOTSET" || mode == "VALID") {
                REQUIRE(g.pb == pb && g.pe == pe);
                if (in + pb + pe >= eff) REQUIRE(g.out == fits(in + pb + pe)); else REQUIRE(g.out <= 0);
            } else {
                REQUIRE(g.out == (in + s - 1) / s && g.pb >= 0 && g.pe >= 0 && g.out == fits(in + g.pb + g.pe));
                REQUIRE(mode == "SAME_UPPER" ? (g.pe == g.pb || g.pe == g.pb + 1) : (g.pb == g.pe || g.pb == g.pe + 1));
                REQUIRE(g.pb + g.pe == std::max<int64_t>(0, (g.out - 1) * s + eff - in));   // the least padding that makes room for the last window
            }
            n++;
        }
        // transposed: input i, tap t lands on i * s + t * d of the unpadded result
        int64_t reach = 0;
        for (int64_t i = 0; i < in; i++) for (int64_t t = 0; t < k; t++) reach = std::max(reach, i * s + t * d + 1);
        for (int64_t opad = 0; opad <= 1; opad++) {
            for (int64_t pb = 0; pb <= 2; pb++) for (int64_t pe = 0; pe <= 2; pe++, n++) {
                const ConvDim g = convtr_dim(in, k, s, d, pb, pe, opad, false, 0, "NOTSET");
                REQUIRE(g.out == reach - pb - pe + opad && g.pb == pb && g.pe == pe);
            }
            for (const char* m : {"SAME_UPPER", "SAME_LOWER"}) {
                const ConvDim g = convtr_dim(in, k, s, d, 1, 1, opad, false, 0, m);
                REQUIRE(g.out == in * s && g.pb + g.pe == std::max<int64_t>(0, reach + opad - g.out));
                REQUIRE(std::string(m) == "SAME_UPPER" ? g.pb == (g.pb + g.pe) / 2 : g.pe == (g.pb + g.pe) / 2);
                n++;
            }
        }
        for (int64_t want = std::max<int64_t>(1, reach - 2); want <= reach + 1; want++) for (const char* m : {"NOTSET", "SAME_UPPER", "SAME_LOWER"}) {
            const ConvDim g = convtr_dim(in, k, s, d, 2, 2, 0, true, want, m);   // output_shape wins over the pads given
            const int64_t tot = std::max<int64_t>(0, reach - want);
            REQUIRE(g.out == want && g.pb + g.pe == tot && g.pb == (std::string(m) == "SAME_UPPER" ? tot / 2 : tot - tot / 2));
            n++;
        }
    }
    REQUIRE(resize_mode_ok("asymmetric", "floor", false) && resize_mode_ok("half_pixel", "round_prefer_floor", true) && !resize_mode_ok("half_pixel", "round_prefer_floor", false) &&
            resize_mode_ok("pytorch_half_pixel", "floor", true) && !resize_mode_ok("align_corners", "floor", true) && !resize_mode_ok("asymmetric", "ceil", true));
    return n;
}

// Reshape / Flatten / Squeeze / Unsqueeze against the operator definitions spelled out, over every shape of rank 0..3 with extents 0..3
static long check_shape_rules() {
    long n = 0;
    std::vector<Shape> shapes = {{}};
    for (int64_t a = 0; a <= 3; a++) { shapes.push_back({a}); for (int64_t b = 0; b <= 3; b++) { shapes.push_back({a, b}); for (int64_t c = 0; c <= 3; c++) shapes.push_back({a, b, c}); } }
    for (const Shape& in : shapes) {
        const int64_t rank = (int64_t)in.size(), numel = prod(in);
        // Flatten: [d_0 .. d_{a-1}] x [d_a .. d_{r-1}], the axis counted from the end when negative, rank itself allowed
        for (int64_t a = -rank; a <= rank; a++, n++) {
            const int64_t p = a < 0 ? a + rank : a;
            int64_t lo = 1, hi = 1;
            for (int64_t d = 0; d < rank; d++) (d < p ? lo : hi) *= in[(size_t)d];
            REQUIRE(flatten_shape(in, a) == Shape({lo, hi}));
        }
        REQUIRE(refuses([&] { flatten_shape(in, rank + 1); }) && refuses([&] { flatten_shape(in, -rank - 1); }));
        // Squeeze: without axes every extent of 1 goes; with axes exactly those dimensions go (negative ones counted from the end)
        { Shape want; for (auto d : in) if (d != 1) want.push_back(d); REQUIRE(squeeze_shape(in, {}) == want); n++; }
        for (int64_t a = -rank; a < rank; a++) for (int64_t b = a; b < rank; b++, n++) {
            const int64_t pa = a < 0 ? a + rank : a, pb = b < 0 ? b + rank : b;
            Shape want; for (int64_t d = 0; d < rank; d++) if (d != pa && d != pb) want.push_back(in[(size_t)d]);
            REQUIRE(squeeze_shape(in, {a, b}) == want);
        }
        REQUIRE(refuses([&] { squeeze_shape(in, {rank}); }));
        // Unsqueeze: the axes index the output (rank + number of axes); it holds 1 there and the input's extents, in order, elsewhere
        for (int64_t a = -rank - 2; a < rank + 2; a++) for (int64_t b = -rank - 2; b < rank + 2; b++) {
            const int64_t r2 = rank + 2, pa = a < 0 ? a + r2 : a, pb = b < 0 ? b + r2 : b;
            if (pa == pb) continue;
            Shape want; size_t src = 0;
            for (int64_t d = 0; d < r2; d++) want.push_back(d == pa || d == pb ? 1 : in[src++]);
            REQUIRE(unsqueeze_shape(in, {a, b}) == want && squeeze_shape(want, {pa, pb}) == in);
            n++;
        }
        REQUIRE(refuses([&] { unsqueeze_shape(in, {rank + 1}); }));
        // Reshape: 0 copies the input's extent at that position unless allowzero, one -1 takes whatever keeps the element count
        std::vector<Shape> targets = {{-1}, {numel}, {1, -1}, {-1, 1, 1}};
        if (rank >= 1) targets.push_back({0, -1});
        if (rank >= 2) { targets.push_back({-1, 0}); targets.push_back({0, 0, -1}); }
        for (const Shape& t : targets) for (int allowzero = 0; allowzero < 2; allowzero++) {
            Shape want = t;
            int64_t known = 1; int hole = -1;
            for (size_t d = 0; d < want.size(); d++) {
                if (want[d] == 0 && !allowzero) want[d] = in[d];
                if (want[d] == -1) hole = (int)d; else known *= want[d];
            }
            if (hole >= 0) want[(size_t)hole] = known ? numel / known : 0;
            const Shape got = reshape_shape(in, t, allowzero != 0);
            REQUIRE(got == want);
            if (numel > 0 && !allowzero) REQUIRE(prod(got) == numel);   // with positive extents the count is kept whenever the target can be met
            n++;
        }
        REQUIRE(refuses([&] { reshape_shape(in, Shape((size_t)rank + 1, 0), false); }));
    }
    // Split, Tile, reduce and Gather output shapes
    REQUIRE(split_sizes(7, {}, 3) == Shape({3, 3, 1}) && split_sizes(6, {}, 3) == Shape({2, 2, 2}) && split_sizes(6, {1, 2, 3}, 3) == Shape({1, 2, 3}));
    REQUIRE(refuses([] { split_sizes(6, {1, 2}, 2); }) && refuses([] { split_sizes(6, {7, -1}, 2); }) && refuses([] { split_sizes(6, {2, 2, 2}, 2); }));
    REQUIRE(tile_shape({2, 3}, {2, 0}) == Shape({4, 0}) && refuses([] { tile_shape({2, 3}, {2}); }) && refuses([] { tile_shape({2, 3}, {-1, 1}); }));
    REQUIRE(reduce_shape({2, 3, 4}, {0, 2}, true) == Shape({1, 3, 1}) && reduce_shape({2, 3, 4}, {0, 2}, false) == Shape({3}) && reduce_shape({2, 3}, {0, 1}, false) == Shape());
    REQUIRE(gather_shape({3, 4, 5}, {2, 2}, 1) == Shape({3, 2, 2, 5}) && gather_shape({3, 4, 5}, {}, 0) == Shape({4, 5}));
    REQUIRE(refuses([] { checked_numel({2, -1}); }) && refuses([] { checked_numel({int64_t(1) << 40, int64_t(1) << 40}); }) && checked_numel({}) == 1 && checked_numel({3, 0}) == 0);
    REQUIRE(strides_of({2, 3, 4}) == Shape({12, 4, 1}) && strides_of({}) == Shape() && prod({2, 3, 4}, 1) == 12 && prod({2, 3, 4}, 0, 1) == 2);
    return n;
}

// the broadcast walker against nested loops, for every pair of shapes of rank 0..3 with extents 1..3 that broadcast; then the evaluators built on it
static long check_walk() {
    long n = 0;
    std::vector<Shape> shapes = {{}};
    for (int64_t a = 1; a <= 3; a++) { shapes.push_back({a}); for (int64_t b = 1; b <= 3; b++) { shapes.push_back({a, b}); for (int64_t c = 1; c <= 3; c++) shapes.push_back({a, b, c}); } }
    auto pad3 = [](const Shape& s) { Shape p(3 - s.size(), 1); p.insert(p.end(), s.begin(), s.end()); return p; };
    for (const Shape& a : shapes) for (const Shape& b : shapes) {
        const Shape pa = pad3(a), pb = pad3(b);
        bool ok = true;
        for (int d = 0; d < 3; d++) ok = ok && (pa[d] == pb[d] || pa[d] == 1 || pb[d] == 1);
        if (!ok) { REQUIRE(refuses([&] { bshape(a, b); })); continue; }
        const Shape os = bshape(a, b), po = pad3(os);
        for (int d = 0; d < 3; d++) REQUIRE(po[d] == std::max(pa[d], pb[d]));
        REQUIRE(os.size() == std::max(a.size(), b.size()));
        Vals av((size_t)prod(a)), bv((size_t)prod(b));
        for (size_t i = 0; i < av.size(); i++) av[i] = 1.0 + (double)i;
        for (size_t i = 0; i < bv.size(); i++) bv[i] = 100.0 * (1.0 + (double)i);
        const Vals sum = host_binary(B_ADD, av, a, bv, b, os, false), pick = host_where(av, a, av, a, bv, b, os);
        int64_t at = 0;
        for (int64_t i = 0; i < po[0]; i++) for (int64_t j = 0; j < po[1]; j++) for (int64_t k = 0; k < po[2]; k++, at++) {
            const int64_t ia = ((pa[0] == 1 ? 0 : i) * pa[1] + (pa[1] == 1 ? 0 : j)) * pa[2] + (pa[2] == 1 ? 0 : k);
            const int64_t ib = ((pb[0] == 1 ? 0 : i) * pb[1] + (pb[1] == 1 ? 0 : j)) * pb[2] + (pb[2] == 1 ? 0 : k);
            REQUIRE(sum[(size_t)at] == av[(size_t)ia] + bv[(size_t)ib] && pick[(size_t)at] == av[(size_t)ia]);
        }
        REQUIRE(at == (int64_t)sum.size());
        n++;
    }
    // the strided copy: a transpose, a reversed slice and a tile of [2][3] against their index formulas
    const Vals x = {0, 1, 2, 3, 4, 5};
    REQUIRE(host_copy(x, {3, 2}, {1, 3}, nomod(2), 0) == Vals({0, 3, 1, 4, 2, 5}));
    REQUIRE(host_copy(x, {2, 2}, {3, -2}, nomod(2), 2) == Vals({2, 0, 5, 3}));
    REQUIRE(host_copy(x, {4, 3}, {3, 1}, {2, 3}, 0) == Vals({0, 1, 2, 3, 4, 5, 0, 1, 2, 3, 4, 5}));
    // integer Div truncates towards zero and refuses nothing (x / 0 is 0); Mod takes the divisor's sign unless fmod
    REQUIRE(host_binary(B_DIV, {-7, 7, -7, 5}, {4}, {2, -2, -2, 0}, {4}, {4}, true) == Vals({-3, -3, 3, 0}) && host_binary(B_DIV, {-7}, {1}, {2}, {1}, {1}, false) == Vals({-3.5}));
    REQUIRE(apply_binary_d(B_MOD, -7, 3) == 2 && apply_binary_d(B_MOD, 7, -3) == -2 && apply_binary_d(B_MOD, 6, 3) == 0 && apply_binary_d(B_MOD, 5, 0) == 0 && apply_binary_d(B_FMOD, -7, 3) == -1);
    // the host unary subset: integers exactly, Round to even, everything else left to the device
    { Vals v = {-3, 0, 2}; REQUIRE(host_unary(U_SIGN, true, v) && v == Vals({-1, 0, 1})); }
    { Vals v = {0.5, 1.5, 2.5, -0.5}; REQUIRE(host_unary(U_ROUND, false, v) && v == Vals({0, 2, 2, -0.0})); }
    { Vals v = {-3, 0, 2}; REQUIRE(host_unary(U_NOT, true, v) && v == Vals({0, 1, 0})); }
    { Vals v = {1.0}; REQUIRE(!host_unary(U_SIGN, false, v) && !host_unary(U_EXP, true, v) && v == Vals({1.0})); }
    // Concat along the middle axis of [2][.][2], Gather with a negative index, the host reductions
    { Vals o(12, -1.0); host_concat_part(o, {0, 1, 2, 3}, 2, 1, 2, 3, 0); host_concat_part(o, {10, 11, 12, 13, 14, 15, 16, 17}, 2, 2, 2, 3, 1);
      REQUIRE(o == Vals({0, 1, 10, 11, 12, 13, 2, 3, 14, 15, 16, 17})); }
    REQUIRE(host_gather({0, 1, 2, 3, 4, 5}, {-1, 0}, 2, 3, 1) == Vals({2, 0, 5, 3}) && refuses([] { host_gather({0, 1, 2}, {3}, 1, 3, 1); }) && refuses([] { host_gather({0, 1, 2}, {-4}, 1, 3, 1); }));
    REQUIRE(host_reduce(R_PROD, {1, 2, 3, 4, 5, 6}, 2, 3) == Vals({6, 120}) && host_reduce(R_MEAN, {1, 2, 3, 4, 5, 6}, 2, 3) == Vals({2, 5}) && host_reduce(R_MAX, {1, 7, 3, 4}, 1, 4) == Vals({7}) &&
            host_reduce(R_MIN, {1, 7, 3, 4}, 2, 2) == Vals({1, 3}) && host_reduce(R_SUM, {1, 7, 3, 4}, 4, 1) == Vals({1, 7, 3, 4}) && host_reduce_ok(R_SUM) && !host_reduce_ok(R_L2));
    return n;
}

int main() {
    std::printf("axes %ld\n", check_axes());
    std::printf("slice %ld\n", check_slice());
    std::printf("conv %ld\n", check_conv());
    std::printf("shapes %ld\n", check_shape_rules());
    std::printf("walk %ld\n", check_walk());
    return 0;
}
