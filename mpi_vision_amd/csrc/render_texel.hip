// render_texel.hip -- the fused warp + over-composite on a narrow-texel RGBA MPI: one schedule,
// templated on a texel-format trait.  Three formats:
//
//   TexU8   8-bit RGBA (4-B texels), the reference's own test-MPI format (test/rgba_00..09.png;
//           utils.py:324-331 reads images as `t.float() / 255.0`).  Packed layout [P][H+4][W+4]
//           uint32 (RGBA bytes, little-endian: R in bits 0-7): a single view moves a quarter of
//           the float render's HBM bytes.
//   TexF16  half-precision RGBA (8-B texels): an MPI that leaves a network under autocast, RGBA16F /
//           EXR assets.  Packed layout [P][H+4][W+4][4] half (R in the lowest 16 bits of the texel's
//           first word): half the HBM bytes and half the memory.
//
//   TexA32  the alpha channel alone (4-B fp32 texels) of an MPI whose RGB is one constant colour per
//           plane: disparity / depth / coverage maps, plane-index and tint views.  Packed layout
//           [P][H+4][W+4] float -- the u8 layout's geometry, a quarter of the float render's bytes.
//           The colour is a per-plane uniform ([P,3], loaded with the homography) and its taps load
//           nothing: a tap is the plane's colour inside the plane and +0 outside (the zero padding
//           the reference samples), decided from the clamped tap origin the loads use.
//
// All layouts keep mpiv_pack_planes' plane-major order and 2-texel zero border.
//
// Bit-exactness: a tap's channel is converted to the float texel the reference renders -- exactly
// (TexU8: RN(u8/255), u8_unit below; TexF16: v_cvt_f32_f16, subnormal halves are normal floats) --
// and the weights, fma chain and over-operator are render.hip's, so the frame equals
// mpi_render_view_torch(u8.float() / 255) resp. mpi_render_view_torch(mpi.float()) bit for bit.
// The conversion happens when the taps are blended, so a tap in flight costs one (u8) or two (f16)
// VGPRs instead of four.
//
// The trait carries everything the formats differ in: the texel type and its byte width, the
// storage of a horizontal tap pair in flight (NW+NE or SW+SE), how a south and a north pair are
// loaded, the conversion of a pair's channel to float, and (for the pack and float-copy kernels) how
// a texel is gathered from the caller's [H,W,P,4] view and expanded to a float4.
// A format may also carry a per-plane context (Ctx, loaded per plane like the homography and handed
// to chan) and per-tap coverage (kCover: cover() is told which of a pair's columns and whether its
// row lie inside the plane); TexU8 and TexF16 have neither (an empty Ctx, no cover calls).
#include "mpiv_common.hpp"

namespace mpiv {

typedef unsigned u32x4 __attribute__((ext_vector_type(4)));

// RN(x / 255) for x in 0..255: v_cvt_f32_ubyte<k>, then fma(x, hi, x*lo) with hi = RN(1/255) and
// lo = RN(1/255 - hi) -- 2 VALU after the byte conversion, the same value as the IEEE division for
// all 256 inputs (tests/test_u8_gpu.py)
__device__ __forceinline__ float u8_unit(unsigned x) {
    const float f = (float)x;
    const float hi = __builtin_bit_cast(float, 998277249u);   // RN(1/255)  = 0x3B808081
    const float lo = __builtin_bit_cast(float, 2944335615u);  // RN(1/255 - hi)
    return __builtin_fmaf(f, hi, f * lo);
}

// channel c (0..3) of the f16 texel in words (w0, w1)
__device__ __forceinline__ float f16_chan(unsigned w0, unsigned w1, int c) {
    const unsigned w = c < 2 ? w0 : w1;
    return (float)__builtin_bit_cast(_Float16, (unsigned short)((c & 1) ? (w >> 16) : (w & 0xFFFFu)));
}

// Pair loads take the byte offset `off` of the pair's row-above texel (cx, cy) in the padded plane;
// the clamp (cx in [-2, W], cy in [-2, H]) plus the 2-texel border keeps cx + 1 and cy + 1 inside
// the plane.  load_north's `sh`: the lane shares the previous row's south pair and reads nothing
// (an out-of-range offset, which the buffer unit answers with zeros without a memory access).
// chan: channel c (0..3) of the pair's texel at cx (side 0) or cx + 1 (side 1), as a float.
struct TexU8 {
    typedef uint8_t Scalar;  // a channel of the caller's view
    typedef unsigned Texel;
    static constexpr int kBytes = 4;
    static constexpr bool kCover = false;
    struct Ctx {};
    static __device__ __forceinline__ Ctx load_ctx(const float*, int) { return Ctx{}; }
    struct Pair {
        unsigned l, r;  // the texels at cx and cx + 1: two 4-B loads
    };
    static __device__ __forceinline__ Pair load_south(__amdgpu_buffer_rsrc_t r, int off, int row) {
        Pair p;
        p.l = __builtin_bit_cast(unsigned, llvm_raw_buffer_load_f32(r, off + row, 0, 0));
        p.r = __builtin_bit_cast(unsigned, llvm_raw_buffer_load_f32(r, off + row + 4, 0, 0));
        return p;
    }
    static __device__ __forceinline__ Pair load_north(__amdgpu_buffer_rsrc_t r, int off, bool sh) {
        Pair p;  // (kOOB - 4 + 4: the instruction's immediate offset must stay out of range too)
        p.l = __builtin_bit_cast(unsigned, llvm_raw_buffer_load_f32(r, sh ? kOOB : off, 0, 0));
        p.r = __builtin_bit_cast(unsigned, llvm_raw_buffer_load_f32(r, (sh ? kOOB - 4 : off) + 4, 0, 0));
        return p;
    }
    static __device__ __forceinline__ float chan(const Pair& t, int side, int c, const Ctx&) {
        return u8_unit(((side ? t.r : t.l) >> (8 * c)) & 255u);
    }
    // pack fast path: the 4 bytes of a texel in one aligned word
    static __device__ __forceinline__ Texel gather(const uint8_t* src, int64_t sc) {
        if (sc == 1 && ((reinterpret_cast<uintptr_t>(src) & 3) == 0)) return *reinterpret_cast<const unsigned*>(src);
        return (unsigned)src[0] | ((unsigned)src[sc] << 8) | ((unsigned)src[2 * sc] << 16) |
               ((unsigned)src[3 * sc] << 24);
    }
    static __device__ __forceinline__ float4 unpack(Texel t) {
        return make_float4(u8_unit(t & 255u), u8_unit((t >> 8) & 255u), u8_unit((t >> 16) & 255u), u8_unit(t >> 24));
    }
};

struct TexF16 {
    typedef uint16_t Scalar;
    typedef uint2 Texel;
    static constexpr int kBytes = 8;
    static constexpr bool kCover = false;
    struct Ctx {};
    static __device__ __forceinline__ Ctx load_ctx(const float*, int) { return Ctx{}; }
    // A pair is 16 contiguous bytes at an 8-B aligned offset and comes in ONE 16-B buffer load
    // (texel cx in .xy, cx + 1 in .zw) -- half as many gather instructions per plane-sample as the
    // float kernel issues (the measured choice between this and one 8-B load per tap: DESIGN.md §4)
    typedef u32x4 Pair;
    static __device__ __forceinline__ Pair load_south(__amdgpu_buffer_rsrc_t r, int off, int row) {
        return __builtin_bit_cast(u32x4, llvm_raw_buffer_load_v4f32(r, off, row, 0));
    }
    static __device__ __forceinline__ Pair load_north(__amdgpu_buffer_rsrc_t r, int off, bool sh) {
        return __builtin_bit_cast(u32x4, llvm_raw_buffer_load_v4f32(r, sh ? kOOB : off, 0, 0));
    }
    static __device__ __forceinline__ float chan(const Pair& t, int side, int c, const Ctx&) {
        return f16_chan(t[2 * side], t[2 * side + 1], c);
    }
    // pack fast path: the 4 halves of a texel in one aligned 8-B word
    static __device__ __forceinline__ Texel gather(const uint16_t* src, int64_t sc) {
        if (sc == 1 && ((reinterpret_cast<uintptr_t>(src) & 7) == 0)) return *reinterpret_cast<const uint2*>(src);
        return make_uint2((unsigned)src[0] | ((unsigned)src[sc] << 16),
                          (unsigned)src[2 * sc] | ((unsigned)src[3 * sc] << 16));
    }
    static __device__ __forceinline__ float4 unpack(Texel t) {  // (the border's +0 halves become +0 floats)
        return make_float4(f16_chan(t.x, t.y, 0), f16_chan(t.x, t.y, 1), f16_chan(t.x, t.y, 2),
                           f16_chan(t.x, t.y, 3));
    }
};

// Alpha-only fp32 planes under a constant colour per plane.  The alpha taps are the u8 format's
// two 4-B words per row; channel c < 3 of a tap is the plane's colour (Ctx) where the tap lies
// inside the plane and +0 where it does not -- a select, so a colour of -0, Inf or NaN reaches the
// fma chain exactly as the constructed float MPI's texel (colour inside, zero border outside) does.
struct TexA32 {
    typedef float Scalar;
    typedef float Texel;
    static constexpr int kBytes = 4;
    static constexpr bool kCover = true;
    struct Ctx {
        float c[3];  // the plane's colour (wave-uniform)
    };
    static __device__ __forceinline__ Ctx load_ctx(const float* __restrict__ colors, int p) {
        Ctx k;
        k.c[0] = colors[(int64_t)p * 3 + 0];
        k.c[1] = colors[(int64_t)p * 3 + 1];
        k.c[2] = colors[(int64_t)p * 3 + 2];
        return k;
    }
    struct Pair {
        unsigned l, r;  // the alpha words at cx and cx + 1
        bool il, ir;    // the taps lie inside the plane (cover)
    };
    static __device__ __forceinline__ Pair load_south(__amdgpu_buffer_rsrc_t r, int off, int row) {
        const TexU8::Pair a = TexU8::load_south(r, off, row);
        return Pair{a.l, a.r, false, false};
    }
    static __device__ __forceinline__ Pair load_north(__amdgpu_buffer_rsrc_t r, int off, bool sh) {
        const TexU8::Pair a = TexU8::load_north(r, off, sh);
        return Pair{a.l, a.r, false, false};
    }
    // xl / xr: column cx / cx + 1 inside [0, W); y: the pair's row inside [0, H)
    static __device__ __forceinline__ void cover(Pair& t, bool xl, bool xr, bool y) {
        t.il = xl && y;
        t.ir = xr && y;
    }
    static __device__ __forceinline__ float chan(const Pair& t, int side, int c, const Ctx& k) {
        if (c == 3) return __builtin_bit_cast(float, side ? t.r : t.l);
        return (side ? t.ir : t.il) ? k.c[c] : 0.0f;
    }
    // pack: `src` points at the channel that is packed (the caller's alpha)
    static __device__ __forceinline__ Texel gather(const float* src, int64_t) { return *src; }
};

// Coverage of the two pairs of a tap set from its clamped origin (cx in [-2, W], cy in [-2, H]; the
// clamp moves no tap across the plane's edge): column cx is inside iff 0 <= cx <= W-1, column cx + 1
// iff -1 <= cx <= W-2; the north row is cy, the south row cy + 1.
template <class T>
__device__ __forceinline__ void cover_taps(typename T::Pair& n, typename T::Pair& s, int cx, int cy, int W, int H) {
    const bool xl = (unsigned)cx < (unsigned)W, xr = (unsigned)(cx + 1) < (unsigned)W;
    T::cover(n, xl, xr, (unsigned)cy < (unsigned)H);
    T::cover(s, xl, xr, (unsigned)(cy + 1) < (unsigned)H);
}

struct TexGeom {
    int org;          // byte offset of texel (0, 0) in a padded plane
    int row;          // Wp * kBytes
    int plane_bytes;  // (H+4)*(W+4) * kBytes
};

template <class T>
struct TapSetTex {
    typename T::Pair n, s;  // NW+NE and SW+SE texel pairs (0 outside the plane: the zero border)
    float wx, wy;           // fractional offsets; weights formed at blend time
};

// issue_taps_padded for narrow texels (org / row in bytes of the format's padded plane)
template <class T>
__device__ __forceinline__ void issue_taps_tex(__amdgpu_buffer_rsrc_t r, int W, int H, int Wp, int org, int row,
                                               float px, float py, TapSetTex<T>& t) {
    const float fx0 = floorf(px), fy0 = floorf(py);
    t.wx = px - fx0;
    t.wy = py - fy0;
    const int cx = (int)__builtin_amdgcn_fmed3f(fx0, -2.0f, (float)W);
    const int cy = (int)__builtin_amdgcn_fmed3f(fy0, -2.0f, (float)H);
    const int off = (__mul24(cy, Wp) + cx) * T::kBytes + org;  // >= 0, <= plane bytes - row - 2 texels
    t.n = T::load_north(r, off, false);
    t.s = T::load_south(r, off, row);
    if constexpr (T::kCover) cover_taps<T>(t.n, t.s, cx, cy, W, H);
}

// blend_taps with the same weight products (issue_taps_padded) and fma chain
template <class T>
__device__ __forceinline__ f32x4 blend_taps_tex(const TapSetTex<T>& t, const typename T::Ctx& kc) {
    const float ex = 1.0f - t.wx, sy = 1.0f - t.wy;
    const float nw = sy * ex, ne = sy * t.wx, sw = t.wy * ex, se = t.wy * t.wx;
    f32x4 o;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        float acc = T::chan(t.n, 0, k, kc) * nw;
        acc = __builtin_fmaf(T::chan(t.n, 1, k, kc), ne, acc);
        acc = __builtin_fmaf(T::chan(t.s, 0, k, kc), sw, acc);
        acc = __builtin_fmaf(T::chan(t.s, 1, k, kc), se, acc);
        o[k] = acc;
    }
    return o;
}

// a pair's two texels as floats
template <class T>
__device__ __forceinline__ void cvt_pair(const typename T::Pair& t, const typename T::Ctx& kc, f32x4& l,
                                         f32x4& r) {
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        l[c] = T::chan(t, 0, c, kc);
        r[c] = T::chan(t, 1, c, kc);
    }
}

// render_rows_pixels on narrow texels: rows y0 .. y0+R-1 of column x, planes outermost, two samples
// in flight (the stretched-MPI route at R = 2, the guarded path of every route; R = 8: vertical
// halo reuse)
template <class T, bool CT, bool GUARD, int R>
__device__ __forceinline__ void render_tex_pixels(const typename T::Texel* __restrict__ planes, int64_t plane_stride,
                                                  const RenderGeom& g, const TexGeom& tg, int p_begin, int p_end,
                                                  int back, const float* __restrict__ hv,
                                                  const float* __restrict__ colors, int x, int y0, float* cr,
                                                  float* cg, float* cb, float* tt) {
    static_assert(R % 2 == 0, "R must be even");
    const float fx = (float)x;
    const bool replace_first = !CT || back;
    const int last = p_end - 1;
    auto hom = [&](int p) { return load_hom(hv + (int64_t)(p < last ? p : last) * 9); };
    auto ctx = [&](int p) { return T::load_ctx(colors, p < last ? p : last); };
    auto issue = [&](int p, int k, const Hom9& h, TapSetTex<T>& ts) {
        const int q = p < last ? p : last;
        float px, py;
        render_pos_fast<GUARD>(h.h, fx, (float)(y0 + k), g, px, py);
        issue_taps_tex<T>(make_rsrc(planes + (int64_t)q * plane_stride, tg.plane_bytes), g.W, g.H, g.Wp, tg.org,
                          tg.row, px, py, ts);
    };
    auto consume = [&](const TapSetTex<T>& ts, const typename T::Ctx& kc, int k, bool first) {
        const f32x4 s = blend_taps_tex<T>(ts, kc);
        const float a = first ? 1.0f : s[3];
        const float om = 1.0f - a;
        cr[k] = over(s[0], a, om, cr[k]);
        cg[k] = over(s[1], a, om, cg[k]);
        cb[k] = over(s[2], a, om, cb[k]);
        if (CT) tt[k] = tt[k] * om;
    };
    TapSetTex<T> A, B;
    Hom9 h = hom(p_begin), hn = hom(p_begin + 1);
    typename T::Ctx kc = ctx(p_begin), kn = ctx(p_begin + 1);  // the colours of the plane consumed / the next
    issue(p_begin, 0, h, A);
    for (int p = p_begin; p < p_end; ++p) {
        const bool first = replace_first && p == p_begin;
#pragma unroll
        for (int k = 0; k < R; k += 2) {  // A holds (p, k)
            issue(p, k + 1, h, B);
            __builtin_amdgcn_sched_barrier(0);
            consume(A, kc, k, first);
            if (k + 2 < R)
                issue(p, k + 2, h, A);
            else
                issue(p + 1, 0, hn, A);  // past the end: the last plane again (cached, unused)
            __builtin_amdgcn_sched_barrier(0);
            consume(B, kc, k + 1, first);
        }
        h = hn;
        hn = hom(p + 2);
        kc = kn;
        kn = ctx(p + 2);
    }
}

// The same with vertical tap reuse (render.hip render_rows_vs_pixels on narrow texels): row k's
// north pair is row k-1's south pair (same clamped offset + one padded row: the same memory
// words) -- and so are its CONVERTED values, so a continuing row loads one pair and converts 8
// channels instead of 16 (the u8 -> RN(u8/255) conversion is most of the u8 kernel's VALU).  The
// north pair is gathered only when some lane of the wave does not continue (wave-uniform branch).
// D > 2: a ring of D rows in flight (row k + D - 1 issued while row k blends, running on into the
// next planes; the plane loop is unrolled by D / R when D > R so ring positions stay static).  At
// one view the launch has 4 waves per SIMD (R = 4), so the loads each wave keeps in flight are what
// hides HBM latency.
// CS: a column-separable view (render.hip ColSet): px, the x weight and the tap column once per
// plane, at the first row the plane issues.
template <class T, bool CT, bool GUARD, int R, int D = 2, bool CS = false>
__device__ __forceinline__ void render_tex_vs_pixels(const typename T::Texel* __restrict__ planes,
                                                     int64_t plane_stride, const RenderGeom& g, const TexGeom& tg,
                                                     int p_begin, int p_end, int back, const float* __restrict__ hv,
                                                     const float* __restrict__ colors, int x, int y0, float* cr,
                                                     float* cg, float* cb, float* tt) {
    static_assert(R % 2 == 0, "R must be even");
    struct Row {
        typename T::Pair n, s;  // NW+NE (own, when not shared) and SW+SE texel pairs
        float wx, wy;
        int off;
        bool sh, own;
    };
    const float fx = (float)x;
    const bool replace_first = !CT || back;
    const int last = p_end - 1;
    auto hom = [&](int p) { return load_hom(hv + (int64_t)(p < last ? p : last) * 9); };
    auto ctx = [&](int p) { return T::load_ctx(colors, p < last ? p : last); };
    static_assert(!CS || !GUARD, "the column set shares one proven division");
    [[maybe_unused]] ColSet col;  // CS: the plane being issued (can_share is false at a plane's first row)
    [[maybe_unused]] int ccx = 0;  // kCover: the tap column cx (CS: of the plane being issued)
    auto issue = [&](int p, int k, const Hom9& h, int prev_off, bool can_share, Row& t) {
        const int q = p < last ? p : last;
        float py;
        int off;
        if constexpr (CS) {
            if (!can_share) {
                col = col_setup<T::kBytes>(h.h, fx, (float)y0, g, tg.org);
                if constexpr (T::kCover) ccx = (col.coff - tg.org) / T::kBytes;  // exact: coff = cx * kBytes + org
            }
            py = col_row_py(h.h, fx, (float)(y0 + k), col, g);
            t.wx = col.wx;
        } else {
            float px;
            render_pos_fast<GUARD>(h.h, fx, (float)(y0 + k), g, px, py);
            const float fx0 = floorf(px);
            t.wx = px - fx0;
            off = (int)__builtin_amdgcn_fmed3f(fx0, -2.0f, (float)g.W);  // cx
            if constexpr (T::kCover) ccx = off;
        }
        const float fy0 = floorf(py);
        t.wy = py - fy0;
        const int cy = (int)__builtin_amdgcn_fmed3f(fy0, -2.0f, (float)g.H);
        if constexpr (CS)
            off = __mul24(cy, tg.row) + col.coff;  // (cy*Wp + cx)*kBytes + org; tg.row < kColsepMaxPitch (render.hip)
        else
            off = (__mul24(cy, g.Wp) + off) * T::kBytes + tg.org;
        t.off = off;
        t.sh = can_share && off == prev_off + tg.row;
        const __amdgpu_buffer_rsrc_t r = make_rsrc(planes + (int64_t)q * plane_stride, tg.plane_bytes);
        t.s = T::load_south(r, off, tg.row);
        t.own = __builtin_amdgcn_ballot_w64(!t.sh) != 0;
        if (t.own)  // wave-uniform: some lane needs its own north pair
            t.n = T::load_north(r, off, t.sh);
        // (a shared north pair is the previous row's south pair, coverage included: the same texels)
        if constexpr (T::kCover) cover_taps<T>(t.n, t.s, ccx, cy, g.W, g.H);
    };
    // pc, pd: the previous row's converted south taps; sc, sd: this row's (out)
    auto consume = [&](const Row& t, const typename T::Ctx& kc, const f32x4& pc, const f32x4& pd, int k, bool first,
                       f32x4& sc, f32x4& sd) {
        cvt_pair<T>(t.s, kc, sc, sd);
        f32x4 na = pc, nb = pd;
        if (t.own) {
            asm volatile("");  // a real wave-uniform branch (render.hip MPIV_VS_ASMBR)
            f32x4 ua, ub;
            cvt_pair<T>(t.n, kc, ua, ub);
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                na[c] = t.sh ? pc[c] : ua[c];
                nb[c] = t.sh ? pd[c] : ub[c];
            }
        }
        const float ex = 1.0f - t.wx, sy = 1.0f - t.wy;
        const float nw = sy * ex, ne = sy * t.wx, sw = t.wy * ex, se = t.wy * t.wx;
        f32x4 s;
#pragma unroll
        for (int c = 0; c < 4; ++c) {  // blend_taps_tex's fma chain
            float acc = na[c] * nw;
            acc = __builtin_fmaf(nb[c], ne, acc);
            acc = __builtin_fmaf(sc[c], sw, acc);
            acc = __builtin_fmaf(sd[c], se, acc);
            s[c] = acc;
        }
        const float a = first ? 1.0f : s[3];
        const float om = 1.0f - a;
        cr[k] = over(s[0], a, om, cr[k]);
        cg[k] = over(s[1], a, om, cg[k]);
        cb[k] = over(s[2], a, om, cb[k]);
        if (CT) tt[k] = tt[k] * om;
        asm volatile("" : "+v"(cr[k]), "+v"(cg[k]), "+v"(cb[k]));  // pinned here (render.hip)
        if (CT) asm volatile("" : "+v"(tt[k]));
    };
    f32x4 pc = {0.f, 0.f, 0.f, 0.f}, pd = pc;
    if constexpr (D != 2) {
        static_assert((R % D == 0 || D % R == 0) && D > 2, "ring positions must repeat every plane group");
        constexpr int U = D > R ? D / R : 1;     // planes per unrolled group (static ring positions)
        constexpr int NH = (R + D - 2) / R + 1;  // homographies live at once: planes p .. p+NH-1
        constexpr int AHEAD = D - 1;             // rows issued ahead of the one consumed
        Row ring[D];
        Hom9 hq[NH];
        typename T::Ctx kq[2] = {ctx(p_begin), ctx(p_begin + 1)};  // the plane consumed and the next
#pragma unroll
        for (int j = 0; j < NH; ++j) hq[j] = hom(p_begin + j);
#pragma unroll
        for (int it = 0; it < AHEAD; ++it)
            issue(p_begin + it / R, it % R, hq[it / R], it % R ? ring[(it + D - 1) % D].off : 0, it % R != 0,
                  ring[it % D]);
        for (int p = p_begin; p < p_end; p += U) {
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const int pu = p + u;
                if (U > 1 && pu >= p_end) break;  // wave-uniform: an odd tail plane
                const bool first = replace_first && pu == p_begin;
#pragma unroll
                for (int k = 0; k < R; ++k) {
                    const int it = u * R + k;   // the row consumed now (item of the group)
                    const int ia = it + AHEAD;  // the row issued now: plane pu + dp (past the end: the last plane again)
                    const int dp = ia / R - u, row = ia % R;
                    issue(pu + dp, row, hq[dp], ring[(ia + D - 1) % D].off, row != 0, ring[ia % D]);
                    asm volatile("" ::: "memory");
                    __builtin_amdgcn_sched_barrier(0);
                    f32x4 sc, sd;
                    consume(ring[it % D], kq[0], pc, pd, k, first, sc, sd);
                    pc = sc;
                    pd = sd;
                }
#pragma unroll
                for (int j = 0; j + 1 < NH; ++j) hq[j] = hq[j + 1];
                hq[NH - 1] = hom(pu + NH);
                kq[0] = kq[1];
                kq[1] = ctx(pu + 2);
            }
        }
        return;
    }
    Hom9 h = hom(p_begin), hn = hom(p_begin + 1);
    typename T::Ctx kc = ctx(p_begin), kn = ctx(p_begin + 1);
    Row A, B;
    issue(p_begin, 0, h, 0, false, A);
    for (int p = p_begin; p < p_end; ++p) {
        const bool first = replace_first && p == p_begin;
#pragma unroll
        for (int k = 0; k < R; k += 2) {  // A holds (p, k)
            issue(p, k + 1, h, A.off, true, B);
            asm volatile("" ::: "memory");
            __builtin_amdgcn_sched_barrier(0);
            f32x4 sc, sd;
            consume(A, kc, pc, pd, k, first, sc, sd);
            pc = sc;
            pd = sd;
            if (k + 2 < R)
                issue(p, k + 2, h, B.off, true, A);
            else
                issue(p + 1, 0, hn, 0, false, A);  // past the end: the last plane again (cached, unused)
            asm volatile("" ::: "memory");
            __builtin_amdgcn_sched_barrier(0);
            consume(B, kc, pc, pd, k + 1, first, sc, sd);
            pc = sc;
            pd = sd;
        }
        h = hn;
        hn = hom(p + 2);
        kc = kn;
        kn = ctx(p + 2);
    }
}

// render_rows_kernel's contract on a packed narrow-texel layout (FAST recipe: H, W >= 2): a
// 256-thread block = 64 x 4R tile, XCD-aware (tile, view) order, tile-level division proof; a tile
// where the proof fails runs the per-sample guarded recipe (GUARD); a tile every plane of which
// samples the zero border composites zeros (render.hip tile_dead).
// G: RenderGeom, or RenderGeomT for a target frame of its own size (render.hip): the tiling, the
// bounds and the output index follow the target grid, everything on the sample path the source.
template <class T, bool CT, int R, bool VS, int D, class G>
__device__ __forceinline__ void render_tex_tile(const typename T::Texel* __restrict__ planes, int64_t plane_stride,
                                                const G& g, const TexGeom& tg, int V, int p_begin, int p_end,
                                                int back, const float* __restrict__ homs, float* __restrict__ out,
                                                int colsep, int order, const float* __restrict__ colors = nullptr) {
    constexpr int TY = 4 * R;
    const int tiles_x = (tgt_w(g) + kTileX - 1) / kTileX;
    const int lb = xcd_logical_block(blockIdx.x, gridDim.x);
    const int v = lb % V;
    const int tile = xcd_tile_order(lb / V, (int)gridDim.x / V, tiles_x, order);  // render.hip
    const int tx0 = (tile % tiles_x) * kTileX, ty0 = (tile / tiles_x) * TY;
    const int x = tx0 + (int)(threadIdx.x & (kWave - 1));
    const int y0 = ty0 + (int)(threadIdx.x >> 6) * R;
    const float* hv = homs + (int64_t)v * g.P * 9;
    bool ok = true, dd = true, cs = true;
    {
        const float x0 = (float)tx0, x1 = (float)min(tx0 + kTileX - 1, tgt_w(g) - 1);
        const float fy0 = (float)ty0, fy1 = (float)min(ty0 + TY - 1, tgt_h(g) - 1);
        for (int p = p_begin + (int)threadIdx.x; p < p_end; p += 256) {
            const float* hp = hv + (int64_t)p * 9;
            const bool safe = div2_rect_safe(hp, x0, x1, fy0, fy1);
            ok = ok && safe;
            dd = dd && safe && tile_dead(hp, x0, x1, fy0, fy1, g);
            cs = cs && hp[1] == 0.0f && hp[7] == 0.0f;  // both signed zeros; NaN fails
        }
    }
    const bool proven = __syncthreads_and(ok);
    const bool dead = __syncthreads_and(dd);
    // column-separable view (render.hip ColSet; colsep and the pitch bound as render_rows_kernel's)
    bool sep = false;
    if constexpr (VS)
        sep = tg.row < kColsepMaxPitch && (colsep > 0 || (colsep == 0 && __syncthreads_and(cs)));
    if (x >= tgt_w(g) || y0 >= tgt_h(g)) return;  // rows past H inside [y0, y0+R) are computed, not stored
    float cr[R], cg[R], cb[R], tt[R];
#pragma unroll
    for (int k = 0; k < R; ++k) {
        cr[k] = -0.0f; cg[k] = -0.0f; cb[k] = -0.0f; tt[k] = 1.0f;  // render_packed_pixel: plane 0 replaces
    }
    if (dead) {  // every plane samples the zero border over the whole tile (render.hip tile_dead)
        composite_zero<CT>(p_begin, p_end, !CT || back, cr[0], cg[0], cb[0], tt[0]);
#pragma unroll
        for (int k = 1; k < R; ++k) {
            cr[k] = cr[0]; cg[k] = cg[0]; cb[k] = cb[0]; tt[k] = tt[0];
        }
    } else if (proven) {
        if constexpr (VS) {
            if (sep)  // block-uniform
                render_tex_vs_pixels<T, CT, false, R, D, true>(planes, plane_stride, g, tg, p_begin, p_end, back, hv,
                                                               colors, x, y0, cr, cg, cb, tt);
            else
                render_tex_vs_pixels<T, CT, false, R, D>(planes, plane_stride, g, tg, p_begin, p_end, back, hv, colors,
                                                         x, y0, cr, cg, cb, tt);
        } else
            render_tex_pixels<T, CT, false, R>(planes, plane_stride, g, tg, p_begin, p_end, back, hv, colors, x, y0, cr,
                                               cg, cb, tt);
    } else {  // rare (w near 0 over the tile): the guarded recipe two rows at a time (few VGPRs)
#pragma unroll
        for (int k = 0; k < R; k += 2)
            render_tex_pixels<T, CT, true, 2>(planes, plane_stride, g, tg, p_begin, p_end, back, hv, colors, x, y0 + k,
                                              cr + k, cg + k, cb + k, tt + k);
    }
#pragma unroll
    for (int k = 0; k < R; ++k) {
        const int y = y0 + k;
        if (y >= tgt_h(g)) break;
        const int64_t o = ((int64_t)v * tgt_h(g) + y) * tgt_w(g) + x;
        if (CT) {
            reinterpret_cast<float4*>(out)[o] = make_float4(cr[k], cg[k], cb[k], tt[k]);
        } else {
            out[o * 3 + 0] = cr[k];
            out[o * 3 + 1] = cg[k];
            out[o * 3 + 2] = cb[k];
        }
    }
}

// The entry points keep one name per format (route strings, profiles and tools key on them).
template <bool CT, int R, bool VS = false, int D = 2>
__global__ __launch_bounds__(256) void render_u8_kernel(const unsigned* __restrict__ planes, int64_t plane_stride,
                                                        RenderGeom g, TexGeom tg, int V, int p_begin, int p_end,
                                                        int back, const float* __restrict__ homs,
                                                        float* __restrict__ out, int colsep = 0, int order = 0) {
    render_tex_tile<TexU8, CT, R, VS, D>(planes, plane_stride, g, tg, V, p_begin, p_end, back, homs, out, colsep,
                                         order);
}

template <bool CT, int R, bool VS = false, int D = 2>
__global__ __launch_bounds__(256) void render_f16_kernel(const uint2* __restrict__ planes, int64_t plane_stride,
                                                         RenderGeom g, TexGeom tg, int V, int p_begin, int p_end,
                                                         int back, const float* __restrict__ homs,
                                                         float* __restrict__ out, int colsep = 0, int order = 0) {
    render_tex_tile<TexF16, CT, R, VS, D>(planes, plane_stride, g, tg, V, p_begin, p_end, back, homs, out, colsep,
                                          order);
}

// The full composite into a target frame of its own size [V,Ht,Wt,3] (mpiv_render_packed_u8_tgt,
// mpiv_render_packed_f16_tgt; render.hip RenderGeomT).
template <int R, bool VS, int D>
__global__ __launch_bounds__(256) void render_u8_tgt_kernel(const unsigned* __restrict__ planes, int64_t plane_stride,
                                                            RenderGeomT g, TexGeom tg, int V,
                                                            const float* __restrict__ homs, float* __restrict__ out,
                                                            int colsep, int order) {
    render_tex_tile<TexU8, false, R, VS, D>(planes, plane_stride, g, tg, V, 0, g.P, 1, homs, out, colsep, order);
}

template <int R, bool VS, int D>
__global__ __launch_bounds__(256) void render_f16_tgt_kernel(const uint2* __restrict__ planes, int64_t plane_stride,
                                                             RenderGeomT g, TexGeom tg, int V,
                                                             const float* __restrict__ homs, float* __restrict__ out,
                                                             int colsep, int order) {
    render_tex_tile<TexF16, false, R, VS, D>(planes, plane_stride, g, tg, V, 0, g.P, 1, homs, out, colsep, order);
}

// Alpha-only planes under per-plane colours [P,3] (TexA32): the full composite only (no (C, T)
// partials), so the template arguments are the rows per work-item, the reuse and the rows in flight.
template <int R, bool VS = false, int D = 2>
__global__ __launch_bounds__(256) void render_alpha_kernel(const float* __restrict__ planes, int64_t plane_stride,
                                                           RenderGeom g, TexGeom tg, int V,
                                                           const float* __restrict__ colors,
                                                           const float* __restrict__ homs, float* __restrict__ out,
                                                           int colsep = 0, int order = 0) {
    render_tex_tile<TexA32, false, R, VS, D>(planes, plane_stride, g, tg, V, 0, g.P, 1, homs, out, colsep, order,
                                             colors);
}

// Packed narrow planes -> packed float planes (the same padded [P][H+4][W+4] layout as
// mpiv_pack_planes), every channel converted exactly: the texels of the float MPI the reference
// renders (u8.float() / 255, mpi.float()).  The many-view route of both renders: at 125 views per
// launch the float rows kernel (texture path and VALU co-limited) beats the u8 kernel (VALU-bound
// on the per-tap conversion), so a camera path converts its MPI once.
// One texel per work-item: a 4- or 8-B read, a 16-B write.
template <class T>
__global__ __launch_bounds__(256) void unpack_planes_kernel(const typename T::Texel* __restrict__ src,
                                                            float4* __restrict__ dst, int64_t n) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256)
        dst[i] = T::unpack(src[i]);
}

// Counter-based synthetic u8 MPI (synth.hip's hash; bytes = top 8 bits of each channel's
// hash, plane 0 alpha 255), straight into the packed u8 layout: a config-5 shard per GPU.
__global__ __launch_bounds__(256) void synth_packed_u8_kernel(uint32_t seed, int H, int W, int p_begin,
                                                              FastDiv wp_div, unsigned* __restrict__ packed,
                                                              int64_t plane_stride) {
    const int64_t pix = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (pix >= plane_stride) return;
    const int p = p_begin + (int)blockIdx.y;
    const int yp = (int)fast_div((unsigned)pix, wp_div);
    const int y = yp - kPad, x = (int)pix - yp * (int)wp_div.d - kPad;
    unsigned v = 0;
    if ((unsigned)y < (unsigned)H && (unsigned)x < (unsigned)W) {
        const uint32_t hp = synth_mix(seed + 0x9E3779B9u * (uint32_t)(p + 1));
        const uint32_t hx = synth_mix(hp ^ (uint32_t)(y * W + x));
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            const unsigned byte = (c == 3 && p == 0) ? 255u : (synth_mix(hx + 0x85EBCA6Bu * (uint32_t)(c + 1)) >> 24);
            v |= byte << (8 * c);
        }
    }
    packed[(int64_t)blockIdx.y * plane_stride + pix] = v;
}

}  // namespace mpiv
