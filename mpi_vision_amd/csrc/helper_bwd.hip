// helper_bwd.hip -- the adjoints of the two primitives the drop-in pipelines are built from:
// mpiv_grid_sample (bilinear_wrapper_torch / resampler_wrapper_torch, utils.py:104-134, 395-407) and
// mpiv_over_composite (utils.py:136-157), each the reference's CPU autograd to the bit.
//
// (a) grid_bwd_pixel_kernel: one work-item per output pixel.  The position is the forward's
//     (unnormalize(to_grid(c), size/2) and bilinear_setup: the tap set depends on its bits), the taps
//     are masked loads (zero outside the image), and the position gradient is warp_bwd_pixel_kernel's:
//
//       gx = gy = +0;  per c:  tx = fma(se_c - sw_c, n, (ne_c - nw_c) * s);  gx = fma(tx, dout_c, gx)
//                              ty = fma(se_c - ne_c, w, (sw_c - nw_c) * e);  gy = fma(ty, dout_c, gy)
//       gx *= Wi/2;  gy *= Hi/2;  dcoords = (gx * 2, gy * 2)      (the adjoint of [-1,-1] + 2.0 * coords)
//
//     no axis swap: that belongs to the callers that normalise x by H.  When d input is wanted the
//     kernel also writes the position and the nw tap's bucket key for warp_bwd.hip's sort and gather
//     (stage (c) there), which take nothing but positions and keys: `coords` is exactly the arbitrary
//     coordinate field they were written for.
//
// (b) over_bwd_kernel: one work-item per pixel, lanes = consecutive pixels.  With out_0 = rgb_0 and
//     out_i = rgb_i * a_i + out_{i-1} * (1 - a_i) the reference's autograd computes, from g = dout,
//
//       i = P-1 .. 1:  d rgb_i = g * a_i + 0
//                      d a_i   = (S(g * rgb_i) + (-S(g * out_{i-1}))) + 0,   S(x) = (x_0 + x_1) + x_2
//                      g       = g * (1 - a_i)
//       layer 0:       (g, +0)
//
//     every operation one fp32 rounding.  The `+ 0` is autograd's sum of a layer's two zero-padded slice
//     gradients (it turns a -0 into +0); layer 0 has one slice only, so a -0 survives there.  The prefix
//     colours out_{i-1} are needed back to front and the blend cannot be inverted exactly, so the scheme
//     is bwd_chain_kernel's: a forward pass writes the colour before every chunk of kOverChunk layers but
//     the first (whose prefix is rgb_0) into the workspace, [chunk][channel][pixel]; the backward pass walks
//     the chunks back to front and rebuilds a chunk's prefixes in registers.  The last chunk is not part
//     of the forward pass, so every layer is read at most twice; P <= kOverChunk + 1 needs no workspace.
//     A work-item reads only the checkpoints it wrote itself: no block waits on another.
#include "mpiv_common.hpp"

namespace mpiv {

__global__ __launch_bounds__(kWarpThreads) void grid_bwd_pixel_kernel(
    const float* __restrict__ in, ImgStrides s, SweepParams sp, const float* __restrict__ coords, Strides4 cs,
    const float* __restrict__ dout, ImgStrides ds, float* __restrict__ dcoords, float2* __restrict__ pos,
    unsigned* __restrict__ key) {
    const unsigned npix = (unsigned)sp.Ht * (unsigned)sp.Wt;  // < 2^31, checked on the host
    const unsigned pix = blockIdx.x * kWarpThreads + threadIdx.x;
    const int b = blockIdx.y;
    if (pix >= npix) return;
    const int y = (int)(pix / (unsigned)sp.Wt), x = (int)(pix % (unsigned)sp.Wt);
    const float* cp = coords + b * cs.n + y * cs.y + x * cs.x;
    const float px = unnormalize(to_grid(cp[0]), sp.half_ws);
    const float py = unnormalize(to_grid(cp[cs.c]), sp.half_hs);
    const Bilinear bl = bilinear_setup(px, py, sp.Ws, sp.Hs);
    const bool m00 = bl.x0 & bl.y0, m10 = bl.x1 & bl.y0, m01 = bl.x0 & bl.y1, m11 = bl.x1 & bl.y1;
    if (pos != nullptr) {
        const bool has = (bl.x0 | bl.x1) & (bl.y0 | bl.y1);  // a corner inside the image (false for NaN)
        const unsigned nb = (unsigned)(sp.Hs + 1) * (unsigned)(sp.Ws + 1);
        pos[(int64_t)b * npix + pix] = make_float2(px, py);
        key[(int64_t)b * npix + pix] = has ? (unsigned)(bl.iy + 1) * (unsigned)(sp.Ws + 1) + (unsigned)(bl.ix + 1) : nb;
    }
    if (dcoords == nullptr) return;  // (uniform: only d input was asked for)

    const float fx0 = floorf(px), fy0 = floorf(py);
    const float w = px - fx0, e = 1.0f - w, n = py - fy0, sth = 1.0f - n;
    const float* src = in + (int64_t)b * s.b;
    const float* dq = dout + b * ds.b + y * ds.y + x * ds.x;
    float gx = 0.0f, gy = 0.0f;
    for (int c = 0; c < sp.C; ++c) {
        const float ta = ld_img(src, s, bl.ix, bl.iy, c, m00), tb = ld_img(src, s, bl.ix + 1, bl.iy, c, m10);
        const float tc = ld_img(src, s, bl.ix, bl.iy + 1, c, m01), td = ld_img(src, s, bl.ix + 1, bl.iy + 1, c, m11);
        const float d = dq[c * ds.c];
        const float tx = __builtin_fmaf(td - tc, n, (tb - ta) * sth);
        gx = __builtin_fmaf(tx, d, gx);
        const float ty = __builtin_fmaf(td - tb, w, (tc - ta) * e);
        gy = __builtin_fmaf(ty, d, gy);
    }
    gx = gx * sp.half_ws;  // grid_sample's unnormalise multipliers
    gy = gy * sp.half_hs;
    float* o = dcoords + ((int64_t)b * npix + pix) * 2;
    o[0] = gx * 2.0f;
    o[1] = gy * 2.0f;
}

constexpr int kOverChunk = 8;  // layers whose prefix colours a work-item rebuilds in registers

// one RGBA pixel of a layer: a 16-B load where the layout and the layer's own pointer allow it
template <bool VEC>
__device__ __forceinline__ float4 over_ld(const float* __restrict__ l, int64_t chs) {
    if (VEC && (reinterpret_cast<uintptr_t>(l) & 15) == 0) return *reinterpret_cast<const float4*>(l);
    return make_float4(l[0], l[chs], l[2 * chs], l[3 * chs]);
}

template <bool VEC>
__global__ __launch_bounds__(256) void over_bwd_kernel(const float* const* __restrict__ layers, int P, int64_t n,
                                                       int64_t ps, int64_t chs, const float* __restrict__ dout,
                                                       int64_t dps, int64_t dcs, float* __restrict__ dlayers,
                                                       float* __restrict__ ckpt) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int nch = (P - 1 + kOverChunk - 1) / kOverChunk;  // chunks of layers 1 .. P-1
    const float4 l0 = over_ld<VEC>(layers[0] + i * ps, chs);
    // forward: the colour before chunk k (k >= 1), i.e. after layer k * kOverChunk
    {
        float r = l0.x, g = l0.y, b = l0.z;
        const int last = (nch - 1) * kOverChunk;  // (<= 0: no checkpoint)
        for (int p = 1; p <= last; ++p) {
            const float4 l = over_ld<VEC>(layers[p] + i * ps, chs);
            const float om = 1.0f - l.w;
            r = over(l.x, l.w, om, r);
            g = over(l.y, l.w, om, g);
            b = over(l.z, l.w, om, b);
            if (p % kOverChunk == 0) {
                float* c = ckpt + (int64_t)(p / kOverChunk - 1) * 3 * n + i;
                c[0] = r;
                c[n] = g;
                c[2 * n] = b;
            }
        }
    }
    const float* dq = dout + i * dps;
    float gr = dq[0], gg = dq[dcs], gb = dq[2 * dcs];
    for (int k = nch - 1; k >= 0; --k) {
        const int base = 1 + k * kOverChunk, cnt = min(kOverChunk, P - base);
        float r, g, b;
        if (k == 0) {
            r = l0.x, g = l0.y, b = l0.z;
        } else {
            const float* c = ckpt + (int64_t)(k - 1) * 3 * n + i;
            r = c[0], g = c[n], b = c[2 * n];
        }
        float4 L[kOverChunk];
        float pr[kOverChunk], pg[kOverChunk], pb[kOverChunk];  // out_{base+j-1}
#pragma unroll
        for (int j = 0; j < kOverChunk; ++j) {
            if (j < cnt) {
                L[j] = over_ld<VEC>(layers[base + j] + i * ps, chs);
                pr[j] = r, pg[j] = g, pb[j] = b;
                const float om = 1.0f - L[j].w;
                r = over(L[j].x, L[j].w, om, r);
                g = over(L[j].y, L[j].w, om, g);
                b = over(L[j].z, L[j].w, om, b);
            }
        }
#pragma unroll
        for (int j = kOverChunk - 1; j >= 0; --j) {
            if (j < cnt) {
                const float a = L[j].w;
                float4 d;
                d.x = gr * a + 0.0f;
                d.y = gg * a + 0.0f;
                d.z = gb * a + 0.0f;
                const float s_rgb = (gr * L[j].x + gg * L[j].y) + gb * L[j].z;
                const float s_out = (gr * pr[j] + gg * pg[j]) + gb * pb[j];
                d.w = (s_rgb + (-s_out)) + 0.0f;
                const float om = 1.0f - a;
                gr = gr * om;
                gg = gg * om;
                gb = gb * om;
                float* o = dlayers + ((int64_t)(base + j) * n + i) * 4;
                if (VEC) {
                    *reinterpret_cast<float4*>(o) = d;
                } else {
                    o[0] = d.x, o[1] = d.y, o[2] = d.z, o[3] = d.w;
                }
            }
        }
    }
    float* o = dlayers + i * 4;
    if (VEC) {
        *reinterpret_cast<float4*>(o) = make_float4(gr, gg, gb, 0.0f);
    } else {
        o[0] = gr, o[1] = gg, o[2] = gb, o[3] = 0.0f;
    }
}

}  // namespace mpiv
