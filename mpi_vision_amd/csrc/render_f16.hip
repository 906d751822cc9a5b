// render_f16.hip -- the fused warp + over-composite on a half-precision RGBA MPI (8-B texels):
// the format of an MPI that leaves a network under autocast and of RGBA16F / EXR assets.
//
// Packed f16 layout: [P][H+4][W+4][4] half (RGBA order, R in the lowest 16 bits of the texel's
// first word), the same plane-major order and 2-texel zero border as mpiv_pack_planes, 8 B per
// texel instead of 16: a view moves half the HBM bytes and the MPI takes half the memory.
//
// Bit-exactness: half -> float is exact (v_cvt_f32_f16, one instruction per channel; subnormal
// halves are normal floats), and the weights, fma chain and over-operator are render.hip's, so
// the frame equals mpi_render_view_torch(mpi.float()) bit for bit.  The conversion happens when
// the taps are blended, so a tap in flight costs two VGPRs instead of four.
//
// Tap loads: a horizontal tap pair (NW+NE or SW+SE) is 16 contiguous bytes at an 8-B aligned
// offset and comes in ONE 16-B buffer load -- half as many gather instructions per plane-sample
// as the float kernel issues (the measured choice between this and one 8-B load per tap:
// DESIGN.md §4).  The clamp (cx in [-2, W], cy in [-2, H]) plus the 2-texel border keeps cx + 1
// and cy + 1 inside the padded plane, so a pair load never leaves the buffer resource.
#include "mpiv_common.hpp"

namespace mpiv {

typedef unsigned u32x4 __attribute__((ext_vector_type(4)));

// one horizontal tap pair: texels (cx, cy) in .xy and (cx + 1, cy) in .zw
__device__ __forceinline__ u32x4 load_pair_f16(__amdgpu_buffer_rsrc_t r, int off, int soff) {
    return __builtin_bit_cast(u32x4, llvm_raw_buffer_load_v4f32(r, off, soff, 0));
}

// channel c (0..3) of the texel in words (w0, w1)
__device__ __forceinline__ float f16_chan(unsigned w0, unsigned w1, int c) {
    const unsigned w = c < 2 ? w0 : w1;
    return (float)__builtin_bit_cast(_Float16, (unsigned short)((c & 1) ? (w >> 16) : (w & 0xFFFFu)));
}

// the pair's two texels as floats
__device__ __forceinline__ void cvt_pair_f16(const u32x4& t, f32x4& l, f32x4& r) {
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        l[c] = f16_chan(t[0], t[1], c);
        r[c] = f16_chan(t[2], t[3], c);
    }
}

struct TapSetF16 {
    u32x4 n, s;    // NW+NE and SW+SE texel pairs (0 outside the plane: the zero border)
    float wx, wy;  // fractional offsets; weights formed at blend time
};

struct F16Geom {
    int org;          // byte offset of texel (0, 0) in a padded f16 plane
    int row;          // Wp * 8
    int plane_bytes;  // (H+4)*(W+4)*8
};

// issue_taps_padded for 8-B texels (org / row in bytes of the f16 padded plane)
__device__ __forceinline__ void issue_taps_f16(__amdgpu_buffer_rsrc_t r, int W, int H, int Wp, int org, int row,
                                               float px, float py, TapSetF16& t) {
    const float fx0 = floorf(px), fy0 = floorf(py);
    t.wx = px - fx0;
    t.wy = py - fy0;
    const int cx = (int)__builtin_amdgcn_fmed3f(fx0, -2.0f, (float)W);
    const int cy = (int)__builtin_amdgcn_fmed3f(fy0, -2.0f, (float)H);
    const int off = (__mul24(cy, Wp) + cx) * 8 + org;  // >= 0, <= plane bytes - row - 16
    t.n = load_pair_f16(r, off, 0);
    t.s = load_pair_f16(r, off, row);
}

// blend_taps with the same weight products (issue_taps_padded) and fma chain
__device__ __forceinline__ f32x4 blend_taps_f16(const TapSetF16& t) {
    const float ex = 1.0f - t.wx, sy = 1.0f - t.wy;
    const float nw = sy * ex, ne = sy * t.wx, sw = t.wy * ex, se = t.wy * t.wx;
    f32x4 a, b, c, d, o;
    cvt_pair_f16(t.n, a, b);
    cvt_pair_f16(t.s, c, d);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        float acc = a[k] * nw;
        acc = __builtin_fmaf(b[k], ne, acc);
        acc = __builtin_fmaf(c[k], sw, acc);
        acc = __builtin_fmaf(d[k], se, acc);
        o[k] = acc;
    }
    return o;
}

// render_u8_pixels on f16 texels: rows y0 .. y0+R-1 of column x, planes outermost, two samples
// in flight (the stretched-MPI route at R = 2, and the guarded path of every route)
template <bool CT, bool GUARD, int R>
__device__ __forceinline__ void render_f16_pixels(const uint2* __restrict__ planes, int64_t plane_stride,
                                                  const RenderGeom& g, const F16Geom& fg, int p_begin, int p_end,
                                                  int back, const float* __restrict__ hv, int x, int y0, float* cr,
                                                  float* cg, float* cb, float* tt) {
    static_assert(R % 2 == 0, "R must be even");
    const float fx = (float)x;
    const bool replace_first = !CT || back;
    const int last = p_end - 1;
    auto hom = [&](int p) { return load_hom(hv + (int64_t)(p < last ? p : last) * 9); };
    auto issue = [&](int p, int k, const Hom9& h, TapSetF16& ts) {
        const int q = p < last ? p : last;
        float px, py;
        render_pos_fast<GUARD>(h.h, fx, (float)(y0 + k), g, px, py);
        issue_taps_f16(make_rsrc(planes + (int64_t)q * plane_stride, fg.plane_bytes), g.W, g.H, g.Wp, fg.org, fg.row,
                       px, py, ts);
    };
    auto consume = [&](const TapSetF16& ts, int k, bool first) {
        const f32x4 s = blend_taps_f16(ts);
        const float a = first ? 1.0f : s[3];
        const float om = 1.0f - a;
        cr[k] = over(s[0], a, om, cr[k]);
        cg[k] = over(s[1], a, om, cg[k]);
        cb[k] = over(s[2], a, om, cb[k]);
        if (CT) tt[k] = tt[k] * om;
    };
    TapSetF16 A, B;
    Hom9 h = hom(p_begin), hn = hom(p_begin + 1);
    issue(p_begin, 0, h, A);
    for (int p = p_begin; p < p_end; ++p) {
        const bool first = replace_first && p == p_begin;
#pragma unroll
        for (int k = 0; k < R; k += 2) {  // A holds (p, k)
            issue(p, k + 1, h, B);
            __builtin_amdgcn_sched_barrier(0);
            consume(A, k, first);
            if (k + 2 < R)
                issue(p, k + 2, h, A);
            else
                issue(p + 1, 0, hn, A);  // past the end: the last plane again (cached, unused)
            __builtin_amdgcn_sched_barrier(0);
            consume(B, k + 1, first);
        }
        h = hn;
        hn = hom(p + 2);
    }
}

// The same with vertical tap reuse (render_u8_vs_pixels on f16 texels): row k's north pair is
// row k-1's south pair (same clamped offset + one padded row: the same memory words) -- and so
// are its CONVERTED values, so a continuing row loads one pair and converts 8 channels instead
// of 16.  The north pair is gathered only when some lane of the wave does not continue
// (wave-uniform branch).
// D > 2: a ring of D rows in flight (row k + D - 1 issued while row k blends, running on into the
// next planes; the plane loop is unrolled by D / R when D > R so ring positions stay static).
// CS: a column-separable view (render.hip ColSet): px, the x weight and the tap column once per
// plane, at the first row the plane issues.
template <bool CT, bool GUARD, int R, int D = 2, bool CS = false>
__device__ __forceinline__ void render_f16_vs_pixels(const uint2* __restrict__ planes, int64_t plane_stride,
                                                     const RenderGeom& g, const F16Geom& fg, int p_begin, int p_end,
                                                     int back, const float* __restrict__ hv, int x, int y0, float* cr,
                                                     float* cg, float* cb, float* tt) {
    static_assert(R % 2 == 0, "R must be even");
    struct RowF16 {
        u32x4 n, s;  // NW+NE (own, when not shared) and SW+SE texel pairs
        float wx, wy;
        int off;
        bool sh, own;
    };
    const float fx = (float)x;
    const bool replace_first = !CT || back;
    const int last = p_end - 1;
    auto hom = [&](int p) { return load_hom(hv + (int64_t)(p < last ? p : last) * 9); };
    static_assert(!CS || !GUARD, "the column set shares one proven division");
    [[maybe_unused]] ColSet col;  // CS: the plane being issued (can_share is false at a plane's first row)
    auto issue = [&](int p, int k, const Hom9& h, int prev_off, bool can_share, RowF16& t) {
        const int q = p < last ? p : last;
        float py;
        int off;
        if constexpr (CS) {
            if (!can_share) col = col_setup<8>(h.h, fx, (float)y0, g, fg.org);
            py = col_row_py(h.h, fx, (float)(y0 + k), col, g);
            t.wx = col.wx;
        } else {
            float px;
            render_pos_fast<GUARD>(h.h, fx, (float)(y0 + k), g, px, py);
            const float fx0 = floorf(px);
            t.wx = px - fx0;
            off = (int)__builtin_amdgcn_fmed3f(fx0, -2.0f, (float)g.W);  // cx
        }
        const float fy0 = floorf(py);
        t.wy = py - fy0;
        const int cy = (int)__builtin_amdgcn_fmed3f(fy0, -2.0f, (float)g.H);
        if constexpr (CS)
            off = __mul24(cy, g.Wp) * 8 + col.coff;  // the same integer: (cy*Wp + cx)*8 + org
        else
            off = (__mul24(cy, g.Wp) + off) * 8 + fg.org;
        t.off = off;
        t.sh = can_share && off == prev_off + fg.row;
        const __amdgpu_buffer_rsrc_t r = make_rsrc(planes + (int64_t)q * plane_stride, fg.plane_bytes);
        t.s = load_pair_f16(r, off, fg.row);
        t.own = __builtin_amdgcn_ballot_w64(!t.sh) != 0;
        if (t.own)  // wave-uniform: some lane needs its own north pair
            t.n = load_pair_f16(r, t.sh ? kOOB : off, 0);
    };
    // pc, pd: the previous row's converted south taps; sc, sd: this row's (out)
    auto consume = [&](const RowF16& t, const f32x4& pc, const f32x4& pd, int k, bool first, f32x4& sc,
                       f32x4& sd) {
        cvt_pair_f16(t.s, sc, sd);
        f32x4 na = pc, nb = pd;
        if (t.own) {
            asm volatile("");  // a real wave-uniform branch (render.hip MPIV_VS_ASMBR)
            f32x4 ua, ub;
            cvt_pair_f16(t.n, ua, ub);
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
        for (int c = 0; c < 4; ++c) {  // blend_taps_f16's fma chain
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
        RowF16 T[D];
        Hom9 hq[NH];
#pragma unroll
        for (int j = 0; j < NH; ++j) hq[j] = hom(p_begin + j);
#pragma unroll
        for (int it = 0; it < AHEAD; ++it)
            issue(p_begin + it / R, it % R, hq[it / R], it % R ? T[(it + D - 1) % D].off : 0, it % R != 0, T[it % D]);
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
                    issue(pu + dp, row, hq[dp], T[(ia + D - 1) % D].off, row != 0, T[ia % D]);
                    asm volatile("" ::: "memory");
                    __builtin_amdgcn_sched_barrier(0);
                    f32x4 sc, sd;
                    consume(T[it % D], pc, pd, k, first, sc, sd);
                    pc = sc;
                    pd = sd;
                }
#pragma unroll
                for (int j = 0; j + 1 < NH; ++j) hq[j] = hq[j + 1];
                hq[NH - 1] = hom(pu + NH);
            }
        }
        return;
    }
    Hom9 h = hom(p_begin), hn = hom(p_begin + 1);
    RowF16 A, B;
    issue(p_begin, 0, h, 0, false, A);
    for (int p = p_begin; p < p_end; ++p) {
        const bool first = replace_first && p == p_begin;
#pragma unroll
        for (int k = 0; k < R; k += 2) {  // A holds (p, k)
            issue(p, k + 1, h, A.off, true, B);
            asm volatile("" ::: "memory");
            __builtin_amdgcn_sched_barrier(0);
            f32x4 sc, sd;
            consume(A, pc, pd, k, first, sc, sd);
            pc = sc;
            pd = sd;
            if (k + 2 < R)
                issue(p, k + 2, h, B.off, true, A);
            else
                issue(p + 1, 0, hn, 0, false, A);  // past the end: the last plane again (cached, unused)
            asm volatile("" ::: "memory");
            __builtin_amdgcn_sched_barrier(0);
            consume(B, pc, pd, k + 1, first, sc, sd);
            pc = sc;
            pd = sd;
        }
        h = hn;
        hn = hom(p + 2);
    }
}

// render_u8_kernel's contract on the packed f16 layout (FAST recipe: H, W >= 2): a 256-thread
// block = 64 x 4R tile, XCD-aware (tile, view) order, tile-level division proof; a tile where the
// proof fails runs the per-sample guarded recipe (GUARD); a tile every plane of which samples
// the zero border composites zeros (render.hip tile_dead).
template <bool CT, int R, bool VS = false, int D = 2>
__global__ __launch_bounds__(256) void render_f16_kernel(const uint2* __restrict__ planes, int64_t plane_stride,
                                                         RenderGeom g, F16Geom fg, int V, int p_begin, int p_end,
                                                         int back, const float* __restrict__ homs,
                                                         float* __restrict__ out, int colsep = 0, int order = 0) {
    constexpr int TY = 4 * R;
    const int tiles_x = (g.W + kTileX - 1) / kTileX;
    const int lb = xcd_logical_block(blockIdx.x, gridDim.x);
    const int v = lb % V;
    const int tile = xcd_tile_order(lb / V, (int)gridDim.x / V, tiles_x, order);  // render.hip
    const int tx0 = (tile % tiles_x) * kTileX, ty0 = (tile / tiles_x) * TY;
    const int x = tx0 + (int)(threadIdx.x & (kWave - 1));
    const int y0 = ty0 + (int)(threadIdx.x >> 6) * R;
    const float* hv = homs + (int64_t)v * g.P * 9;
    bool ok = true, dd = true, cs = true;
    {
        const float x0 = (float)tx0, x1 = (float)min(tx0 + kTileX - 1, g.W - 1);
        const float fy0 = (float)ty0, fy1 = (float)min(ty0 + TY - 1, g.H - 1);
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
    // column-separable view (render.hip ColSet; colsep as render_rows_kernel's)
    bool sep = false;
    if constexpr (VS) sep = colsep > 0 || (colsep == 0 && __syncthreads_and(cs));
    if (x >= g.W || y0 >= g.H) return;  // rows past H inside [y0, y0+R) are computed, not stored
    float cr[R], cg[R], cb[R], tt[R];
#pragma unroll
    for (int k = 0; k < R; ++k) {
        cr[k] = -0.0f; cg[k] = -0.0f; cb[k] = -0.0f; tt[k] = 1.0f;  // render_packed_pixel: plane 0 replaces
    }
    if (dead) {
        composite_zero<CT>(p_begin, p_end, !CT || back, cr[0], cg[0], cb[0], tt[0]);
#pragma unroll
        for (int k = 1; k < R; ++k) {
            cr[k] = cr[0]; cg[k] = cg[0]; cb[k] = cb[0]; tt[k] = tt[0];
        }
    } else if (proven) {
        if constexpr (VS) {
            if (sep)  // block-uniform
                render_f16_vs_pixels<CT, false, R, D, true>(planes, plane_stride, g, fg, p_begin, p_end, back, hv, x,
                                                            y0, cr, cg, cb, tt);
            else
                render_f16_vs_pixels<CT, false, R, D>(planes, plane_stride, g, fg, p_begin, p_end, back, hv, x, y0,
                                                      cr, cg, cb, tt);
        } else
            render_f16_pixels<CT, false, R>(planes, plane_stride, g, fg, p_begin, p_end, back, hv, x, y0, cr, cg, cb,
                                            tt);
    } else {  // rare (w near 0 over the tile): the guarded recipe two rows at a time (few VGPRs)
#pragma unroll
        for (int k = 0; k < R; k += 2)
            render_f16_pixels<CT, true, 2>(planes, plane_stride, g, fg, p_begin, p_end, back, hv, x, y0 + k, cr + k,
                                           cg + k, cb + k, tt + k);
    }
#pragma unroll
    for (int k = 0; k < R; ++k) {
        const int y = y0 + k;
        if (y >= g.H) break;
        const int64_t o = ((int64_t)v * g.H + y) * g.W + x;
        if (CT) {
            reinterpret_cast<float4*>(out)[o] = make_float4(cr[k], cg[k], cb[k], tt[k]);
        } else {
            out[o * 3 + 0] = cr[k];
            out[o * 3 + 1] = cg[k];
            out[o * 3 + 2] = cb[k];
        }
    }
}

// [H,W,P,4] half (element strides y, x, p, c) -> packed f16 planes [P][H+4][W+4] 8-B texels,
// zero border.  A block moves 64 padded pixels x 16 planes through LDS (reads: a pixel's 16
// planes are 128 contiguous bytes; writes: 64 texels = 512 B per plane).
__global__ __launch_bounds__(256) void pack_planes_f16_kernel(const uint16_t* __restrict__ mpi, NativeStrides s, int H,
                                                              int W, int P, FastDiv wp_div, uint2* __restrict__ packed,
                                                              int64_t plane_stride) {
    __shared__ uint2 tile[kPackPl][kPackPix + 1];
    const int64_t npix = plane_stride;
    const int64_t pix0 = (int64_t)blockIdx.x * kPackPix;
    const int p0 = blockIdx.y * kPackPl;
    for (int k = threadIdx.x; k < kPackPix * kPackPl; k += blockDim.x) {
        const int j = k % kPackPl, i = k / kPackPl;
        const int64_t pix = pix0 + i;
        const int p = p0 + j;
        uint2 val = make_uint2(0u, 0u);
        if (pix < npix && p < P) {
            const int yp = (int)fast_div((unsigned)pix, wp_div);
            const int yy = yp - kPad, xx = (int)pix - yp * (int)wp_div.d - kPad;
            if ((unsigned)yy < (unsigned)H && (unsigned)xx < (unsigned)W) {
                const uint16_t* src = mpi + (int64_t)yy * s.y + (int64_t)xx * s.x + (int64_t)p * s.p;
                if (s.c == 1 && ((reinterpret_cast<uintptr_t>(src) & 7) == 0))
                    val = *reinterpret_cast<const uint2*>(src);
                else
                    val = make_uint2((unsigned)src[0] | ((unsigned)src[s.c] << 16),
                                     (unsigned)src[2 * s.c] | ((unsigned)src[3 * s.c] << 16));
            }
        }
        tile[j][i] = val;
    }
    __syncthreads();
    for (int k = threadIdx.x; k < kPackPix * kPackPl; k += blockDim.x) {
        const int i = k % kPackPix, j = k / kPackPix;
        const int64_t pix = pix0 + i;
        const int p = p0 + j;
        if (pix < npix && p < P) packed[(int64_t)p * plane_stride + pix] = tile[j][i];
    }
}

// Packed f16 planes -> packed float planes (the same padded [P][H+4][W+4] layout as
// mpiv_pack_planes), every channel converted exactly: the texels of the float MPI mpi.float().
// The border's +0 halves become +0 floats.  One texel per work-item: an 8-B read, a 16-B write.
__global__ __launch_bounds__(256) void unpack_planes_f16_kernel(const uint2* __restrict__ src, float4* __restrict__ dst,
                                                                int64_t n) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        const uint2 t = src[i];
        dst[i] = make_float4(f16_chan(t.x, t.y, 0), f16_chan(t.x, t.y, 1), f16_chan(t.x, t.y, 2),
                             f16_chan(t.x, t.y, 3));
    }
}

}  // namespace mpiv
