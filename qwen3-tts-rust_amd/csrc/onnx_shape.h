// onnx_shape.h -- the host-only rules of the ONNX executor (onnx_exec.hip): checked axes, broadcast shapes and strides, the shape rules of the
// data-movement operators, Slice and convolution geometry, and the evaluators of host tensors (std::vector<double>).  Plain C++ with no HIP
// header, so tests/host/onnx_shape_main.cpp holds every rule against a plain restatement under the host sanitizers
// (tests/test_onnx_shape_cpu.py).  Operator semantics follow the public ONNX operator specification [EXT].
#pragma once
#include <algorithm>
#include <array>
#include <cmath>
#include <cstdint>
#include <limits>
#include <stdexcept>
#include <string>
#include <vector>

#ifdef __HIPCC__
#define XS_HD __host__ __device__ __forceinline__
#else
#define XS_HD inline
#endif

namespace q3 {
namespace xs {

struct ShapeError : std::runtime_error { using std::runtime_error::runtime_error; };
#define XS_CHECK(cond, msg) do { if (!(cond)) throw ::q3::xs::ShapeError(std::string(msg) + " (" #cond ") at " __FILE__ ":" + std::to_string(__LINE__)); } while (0)

using Shape = std::vector<int64_t>;

enum UOp { U_RELU, U_SIGMOID, U_TANH, U_EXP, U_LOG, U_SQRT, U_RECIP, U_NEG, U_ABS, U_SIN, U_COS, U_ERF, U_FLOOR, U_CEIL, U_ROUND, U_SIGN, U_ELU,
           U_LEAKY, U_HSIG, U_GELU, U_GELU_TANH, U_SOFTPLUS, U_SELU, U_NOT, U_CLIP, U_IDENT, U_SOFTSIGN, U_HSWISH, U_ISNAN, U_CELU, U_THRELU, U_MISH, U_TAN, U_ATAN, U_SINH, U_COSH, U_LOG1P_EXP_NEG };
enum BOp { B_ADD, B_SUB, B_MUL, B_DIV, B_POW, B_MIN, B_MAX, B_EQ, B_LT, B_GT, B_LE, B_GE, B_AND, B_OR, B_XOR, B_MOD, B_FMOD, B_PRELU, B_IDIV };
enum ROp { R_SUM, R_MEAN, R_MAX, R_MIN, R_PROD, R_L2, R_SUMSQ, R_L1, R_LOGSUMEXP, R_ARGMAX, R_ARGMIN };

// ------------------------------------------------------------------------------------------------------------------ axes, shapes, strides
// the checked normalisation of an axis attribute: [-rank, rank) -> [0, rank); `end_ok` also admits rank itself (Flatten)
inline int64_t axis_of(int64_t a, int64_t rank, const std::string& what, bool end_ok = false) {
    const bool ok = a >= -rank && (a < rank || (end_ok && a == rank));
    if (!ok) throw ShapeError((what.empty() ? std::string() : what + ": ") + "axis out of range (axis " + std::to_string(a) + ", rank " + std::to_string(rank) + ")");
    return a < 0 ? a + rank : a;
}
inline Shape norm_axes(Shape axes, int64_t rank) { // checked, sorted, unique
    for (auto& a : axes) a = axis_of(a, rank, "");
    std::sort(axes.begin(), axes.end());
    axes.erase(std::unique(axes.begin(), axes.end()), axes.end());
    return axes;
}
inline Shape strides_of(const Shape& s) { Shape st(s.size(), 1); for (int d = (int)s.size() - 2; d >= 0; d--) st[(size_t)d] = st[(size_t)d + 1] * s[(size_t)d + 1]; return st; }
inline int64_t prod(const Shape& s, size_t a = 0, size_t b = (size_t)-1) { int64_t n = 1; for (size_t i = a; i < std::min(b, s.size()); i++) n *= s[i]; return n; }
// a shape computed from graph data with a negative dimension or an element count that overflows becomes an error before any buffer is sized from it
inline int64_t checked_numel(const Shape& shape) {
    int64_t n = 1;
    for (auto d : shape) {
        XS_CHECK(d >= 0, "tensor shape has a negative dimension");
        XS_CHECK(!__builtin_mul_overflow(n, d, &n) && n <= ((int64_t)1 << 33), "tensor element count overflows / exceeds 2^33");
    }
    return n;
}
inline Shape bshape(const Shape& a, const Shape& b) {
    const size_t r = std::max(a.size(), b.size());
    Shape o(r);
    for (size_t i = 0; i < r; i++) {
        const int64_t x = i + a.size() >= r ? a[i + a.size() - r] : 1, y = i + b.size() >= r ? b[i + b.size() - r] : 1;
        if (x != y && x != 1 && y != 1) throw ShapeError("shapes do not broadcast");
        o[i] = x == 1 ? y : x;
    }
    return o;
}
inline Shape bstrides(const Shape& in, const Shape& out) { // strides of `in` seen through `out` (0 on broadcast dims)
    Shape st = strides_of(in), o(out.size(), 0);
    for (size_t i = 0; i < in.size(); i++) { const size_t d = out.size() - in.size() + i; o[d] = in[i] == 1 ? 0 : st[i]; }
    return o;
}
inline Shape nomod(size_t r) { return Shape(r, std::numeric_limits<int64_t>::max()); }
// The one host walk over a row-major tensor of shape `os`: f(i, off) for every element i, off[k] = the offset of operand k seen through its
// strides st[k] (0 = broadcast).  `mod` wraps operand 0's index per dimension (the period of Tile; nomod() otherwise).
template <size_t N, typename F>
inline void walk(const Shape& os, const std::array<const Shape*, N>& st, const Shape* mod, F&& f) {
    const int64_t n = prod(os);
    for (int64_t i = 0; i < n; i++) {
        int64_t r = i;
        std::array<int64_t, N> off{};
        for (int d = (int)os.size() - 1; d >= 0; d--) {
            const int64_t q = r / os[(size_t)d], x = r - q * os[(size_t)d];
            for (size_t k = 0; k < N; k++) off[k] += ((mod && k == 0) ? x % (*mod)[(size_t)d] : x) * (*st[k])[(size_t)d];
            r = q;
        }
        f(i, off);
    }
}

// ------------------------------------------------------------------------------------------------------------------ shape rules
inline Shape reshape_shape(const Shape& in, Shape shape, bool allowzero) { // 0 copies the input's dimension (unless allowzero), one -1 takes what is left
    int64_t known = 1; int neg = -1;
    for (size_t d = 0; d < shape.size(); d++) {
        if (shape[d] == 0 && !allowzero) { XS_CHECK(d < in.size(), "Reshape: 0 beyond the input rank"); shape[d] = in[d]; }
        if (shape[d] == -1) neg = (int)d; else known *= shape[d];
    }
    if (neg >= 0) shape[(size_t)neg] = known ? prod(in) / known : 0;
    return shape;
}
inline Shape flatten_shape(const Shape& in, int64_t axis) {
    const size_t a = (size_t)axis_of(axis, (int64_t)in.size(), "Flatten", true);
    return {prod(in, 0, a), prod(in, a)};
}
inline Shape squeeze_shape(const Shape& in, const Shape& axes0) { // no axes: every dimension of 1
    Shape s;
    if (axes0.empty()) { for (auto d : in) if (d != 1) s.push_back(d); return s; }
    const Shape axes = norm_axes(axes0, (int64_t)in.size());
    for (size_t d = 0; d < in.size(); d++) if (!std::binary_search(axes.begin(), axes.end(), (int64_t)d)) s.push_back(in[d]);
    return s;
}
inline Shape unsqueeze_shape(const Shape& in, const Shape& axes0) { // the axes index the OUTPUT
    const int r = (int)(in.size() + axes0.size());
    const Shape axes = norm_axes(axes0, r);
    Shape s;
    size_t src = 0;
    for (int d = 0; d < r; d++) s.push_back(std::binary_search(axes.begin(), axes.end(), (int64_t)d) ? 1 : in[src++]);
    return s;
}
inline Shape split_sizes(int64_t dim, Shape sizes, size_t n_outputs) { // explicit sizes checked; none: equal parts, the last one shorter
    { int64_t tot = 0; for (auto z : sizes) { XS_CHECK(z >= 0, "Split: negative size"); tot += z; } XS_CHECK(sizes.empty() || tot == dim, "Split: sizes do not add up to the axis length"); }
    XS_CHECK(sizes.empty() || sizes.size() <= n_outputs, "Split: more sizes than outputs");
    if (sizes.empty()) {
        const int64_t parts = (int64_t)n_outputs, each = (dim + parts - 1) / parts;
        for (int64_t i = 0; i < parts; i++) sizes.push_back(std::min(each, dim - i * each));
    }
    return sizes;
}
inline Shape tile_shape(const Shape& in, const Shape& rep) {
    XS_CHECK(rep.size() == in.size(), "Tile: repeats has " + std::to_string(rep.size()) + " entries for a rank-" + std::to_string(in.size()) + " tensor");
    Shape os(in.size());
    for (size_t d = 0; d < os.size(); d++) { XS_CHECK(rep[d] >= 0 && rep[d] <= (1 << 24), "Tile: repeat count out of range"); os[d] = in[d] * rep[d]; }
    return os;
}
inline Shape reduce_shape(const Shape& in, const Shape& axes, bool keep) { // axes normalised
    Shape os;
    for (size_t d = 0; d < in.size(); d++) { const bool red = std::binary_search(axes.begin(), axes.end(), (int64_t)d); if (!red) os.push_back(in[d]); else if (keep) os.push_back(1); }
    return os;
}
inline Shape gather_shape(const Shape& x, const Shape& idx, int64_t a) { // a normalised
    Shape os(x.begin(), x.begin() + a);
    os.insert(os.end(), idx.begin(), idx.end());
    os.insert(os.end(), x.begin() + a + 1, x.end());
    return os;
}

// ------------------------------------------------------------------------------------------------------------------ Slice geometry
struct SliceAxis { int64_t count, start, step; }; // the output extent, the first input index, the input step (either sign)
inline SliceAxis slice_axis(int64_t dim, int64_t start, int64_t end, int64_t step) {
    XS_CHECK(step != 0, "Slice step 0");
    if (dim == 0) return {0, 0, step}; // nothing to take (the clamps below would make one element of an empty axis under a negative step)
    int64_t s = start, e = end;
    if (s < 0) s += dim;
    if (e < 0) e += dim;
    if (step > 0) { s = std::max<int64_t>(0, std::min(s, dim)); e = std::max<int64_t>(0, std::min(e, dim)); }
    else { s = std::max<int64_t>(0, std::min(s, dim - 1)); e = std::max<int64_t>(-1, std::min(e, dim - 1)); if (end < -dim) e = -1; }
    const int64_t cnt = step > 0 ? std::max<int64_t>(0, (e - s + step - 1) / step) : std::max<int64_t>(0, (s - e + (-step) - 1) / (-step));
    return {cnt, s, step};
}

// ------------------------------------------------------------------------------------------------------------------ convolution geometry
struct ConvDim { int64_t out, pb, pe; }; // output extent and the begin / end pads in force, for one spatial dimension
inline ConvDim conv_dim(int64_t in, int64_t k, int64_t stride, int64_t dil, int64_t pb, int64_t pe, const std::string& auto_pad) {
    const int64_t eff = (k - 1) * dil + 1;
    ConvDim g{0, pb, pe};
    if (auto_pad == "SAME_UPPER" || auto_pad == "SAME_LOWER") {
        g.out = (in + stride - 1) / stride;
        const int64_t tot = std::max<int64_t>(0, (g.out - 1) * stride + eff - in);
        g.pb = auto_pad == "SAME_UPPER" ? tot / 2 : tot - tot / 2; g.pe = tot - g.pb;
    } else {
        if (auto_pad == "VALID") g.pb = g.pe = 0;
        const int64_t room = in + g.pb + g.pe - eff; // < 0: not one window fits (floor, not truncation: no output instead of one)
        g.out = room >= 0 ? room / stride + 1 : -((-room + stride - 1) / stride) + 1;
    }
    return g;
}
// ConvTranspose: an explicit output_shape or a SAME mode fixes the extent and derives the pads; otherwise the pads fix the extent
inline ConvDim convtr_dim(int64_t in, int64_t k, int64_t stride, int64_t dil, int64_t pb, int64_t pe, int64_t opad, bool has_oshape, int64_t oshape, const std::string& auto_pad) {
    const int64_t eff = (k - 1) * dil + 1;
    ConvDim g{0, pb, pe};
    if (has_oshape || auto_pad == "SAME_UPPER" || auto_pad == "SAME_LOWER") {
        g.out = has_oshape ? oshape : in * stride;
        const int64_t tot = std::max<int64_t>(0, (in - 1) * stride + opad + eff - g.out);
        g.pb = auto_pad == "SAME_UPPER" ? tot / 2 : tot - tot / 2; g.pe = tot - g.pb;
    } else g.out = (in - 1) * stride - pb - pe + eff + opad;
    return g;
}
// k_resize_nearest samples x_in = floor(x_out / scale) (asymmetric + floor).  ONNX defaults to half_pixel + round_prefer_floor, which picks the
// same sample exactly when every scale is a whole number >= 1; any other combination is refused instead of silently resampling differently
inline bool resize_mode_ok(const std::string& ctm, const std::string& nm, bool whole) {
    const bool native = ctm == "asymmetric" && nm == "floor";
    const bool equivalent = whole && (ctm == "half_pixel" || ctm == "pytorch_half_pixel" || ctm == "asymmetric") && (nm == "round_prefer_floor" || nm == "floor");
    return native || equivalent;
}

// ------------------------------------------------------------------------------------------------------------------ host evaluators
XS_HD double apply_binary_d(int op, double x, double y) {
    switch (op) {
        case B_ADD: return x + y;
        case B_SUB: return x - y;
        case B_MUL: return x * y;
        case B_DIV: return x / y;
        case B_IDIV: return y != 0 ? (double)(long long)(x / y) : 0.0; // integer division truncates towards zero
        case B_POW: return pow(x, y);
        case B_MIN: return x < y ? x : y;
        case B_MAX: return x > y ? x : y;
        case B_EQ: return x == y ? 1.0 : 0.0;
        case B_LT: return x < y ? 1.0 : 0.0;
        case B_GT: return x > y ? 1.0 : 0.0;
        case B_LE: return x <= y ? 1.0 : 0.0;
        case B_GE: return x >= y ? 1.0 : 0.0;
        case B_AND: return (x != 0 && y != 0) ? 1.0 : 0.0;
        case B_OR: return (x != 0 || y != 0) ? 1.0 : 0.0;
        case B_XOR: return ((x != 0) != (y != 0)) ? 1.0 : 0.0;
        case B_MOD: { if (y == 0) return 0.0; double r = fmod(x, y); if (r != 0 && ((r < 0) != (y < 0))) r += y; return r; } // sign of the divisor (fmod = 0)
        case B_FMOD: return fmod(x, y);
        case B_PRELU: return x > 0 ? x : x * y;
        default: return x;
    }
}
using Vals = std::vector<double>;
// `ints`: both operands hold integers, so Div truncates
inline Vals host_binary(int op, const Vals& a, const Shape& ashape, const Vals& b, const Shape& bshape_, const Shape& os, bool ints) {
    Vals o((size_t)prod(os));
    const Shape as = bstrides(ashape, os), bs = bstrides(bshape_, os);
    const int hop = (op == B_DIV && ints) ? B_IDIV : op;
    walk<2>(os, {&as, &bs}, nullptr, [&](int64_t i, const std::array<int64_t, 2>& off) { o[(size_t)i] = apply_binary_d(hop, a[(size_t)off[0]], b[(size_t)off[1]]); });
    return o;
}
// the unary operators evaluated on the host: a few on integer tensors (exactly), a few more on any host tensor; everything else goes to the device
inline bool host_unary(int op, bool ints, Vals& v) {
    if (ints && (op == U_NEG || op == U_ABS || op == U_SIGN || op == U_IDENT || op == U_NOT)) {
        for (auto& x : v) x = op == U_NEG ? -x : op == U_ABS ? std::fabs(x) : op == U_SIGN ? (x > 0) - (x < 0) : op == U_NOT ? (x != 0 ? 0 : 1) : x;
        return true;
    }
    if (op == U_FLOOR || op == U_CEIL || op == U_SQRT || op == U_NEG || op == U_ABS || op == U_ROUND || op == U_NOT) {
        for (auto& x : v) x = op == U_FLOOR ? std::floor(x) : op == U_CEIL ? std::ceil(x) : op == U_SQRT ? std::sqrt(x) : op == U_NEG ? -x : op == U_ABS ? std::fabs(x)
                               : op == U_ROUND ? std::nearbyint(x) : (x != 0 ? 0 : 1);
        return true;
    }
    return false;
}
inline Vals host_where(const Vals& c, const Shape& cshape, const Vals& a, const Shape& ashape, const Vals& b, const Shape& bshape_, const Shape& os) {
    Vals o((size_t)prod(os));
    const Shape cs = bstrides(cshape, os), as = bstrides(ashape, os), bs = bstrides(bshape_, os);
    walk<3>(os, {&cs, &as, &bs}, nullptr, [&](int64_t i, const std::array<int64_t, 3>& off) { o[(size_t)i] = c[(size_t)off[0]] != 0 ? a[(size_t)off[1]] : b[(size_t)off[2]]; });
    return o;
}
// general strided copy (transpose / slice / expand / tile): out[i] = in[ioff + sum_d (index_d % imod_d) * istride_d]
inline Vals host_copy(const Vals& in, const Shape& oshape, const Shape& istride, const Shape& imod, int64_t ioff) {
    Vals o((size_t)prod(oshape));
    walk<1>(oshape, {&istride}, &imod, [&](int64_t i, const std::array<int64_t, 1>& off) { o[(size_t)i] = in[(size_t)(ioff + off[0])]; });
    return o;
}
// one part [outer][part][inner] of a concatenation into out [outer][total][inner] at axis offset `at`
inline void host_concat_part(Vals& out, const Vals& in, int64_t outer, int64_t part, int64_t inner, int64_t total, int64_t at) {
    for (int64_t o = 0; o < outer; o++) for (int64_t p = 0; p < part; p++) for (int64_t q = 0; q < inner; q++)
        out[(size_t)((o * total + at + p) * inner + q)] = in[(size_t)((o * part + p) * inner + q)];
}
inline Vals host_gather(const Vals& x, const Vals& idx, int64_t outer, int64_t dim, int64_t inner) {
    const int64_t nidx = (int64_t)idx.size();
    Vals o((size_t)(outer * nidx * inner));
    for (int64_t o_ = 0; o_ < outer; o_++) for (int64_t j = 0; j < nidx; j++) {
        int64_t k = (int64_t)idx[(size_t)j]; if (k < 0) k += dim;
        XS_CHECK(k >= 0 && k < dim, "Gather index out of range");
        for (int64_t q = 0; q < inner; q++) o[(size_t)((o_ * nidx + j) * inner + q)] = x[(size_t)((o_ * dim + k) * inner + q)];
    }
    return o;
}
inline bool host_reduce_ok(int r) { return r == R_SUM || r == R_PROD || r == R_MAX || r == R_MIN || r == R_MEAN; }
inline Vals host_reduce(int r, const Vals& p, int64_t rows, int64_t cols) { // p = [rows][cols], the reduced axes last (shape arithmetic: ReduceProd of a shape, ...)
    Vals o((size_t)rows);
    for (int64_t i = 0; i < rows; i++) {
        double acc = r == R_PROD ? 1 : r == R_MAX ? -INFINITY : r == R_MIN ? INFINITY : 0;
        for (int64_t c = 0; c < cols; c++) { const double v = p[(size_t)(i * cols + c)]; acc = r == R_PROD ? acc * v : r == R_MAX ? std::max(acc, v) : r == R_MIN ? std::min(acc, v) : acc + v; }
        o[(size_t)i] = r == R_MEAN ? acc / (double)cols : acc;
    }
    return o;
}

} // namespace xs
} // namespace q3
