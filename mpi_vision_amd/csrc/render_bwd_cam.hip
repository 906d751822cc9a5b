// render_bwd_cam.hip -- d(render)/d(homographies): the camera half of the render's adjoint
// (autograd of mpi_render_view_torch, utils.py:267-294, w.r.t. the 3x3 plane homographies; the
// chain from there to tgt_pose, planes and intrinsics is nine numbers per plane and stays in
// torch on the host, _host.render_homographies_autograd).
//
// The over-composite's adjoint is already paid for: bwd_chain_*_kernel (render_bwd.hip) leaves
// d sample (d rgb, d a) of every plane-pixel in BwdWs::ds.  What remains per plane-sample is the
// adjoint of the bilinear sampler w.r.t. the sample position, of grid_sample's unnormalise, of
// the reference's (swapped) normalisation and of the projective division:
//
//   gx = gy = +0;  for c = 0..3:  tx = fma(se_c - sw_c, n, (ne_c - nw_c) * s);  gx = fma(tx, ds_c, gx)
//                                 ty = fma(se_c - ne_c, w, (sw_c - nw_c) * e);  gy = fma(ty, ds_c, gy)
//   gx *= W/2;  gy *= H/2;  ax = (gx * 2) / (H-1);  ay = (gy * 2) / (W-1)
//   wd = (w3 == 0) ? w3 + 1e-8f : w3;   du = ax / wd;  dv = ay / wd
//   dw = (-ax * ((u / wd) / wd)) + (-ay * ((v / wd) / wd))
//
// (every line one fp32 rounding, the divisions IEEE: the reference's per-sample gradient of
// transform_points_torch's output, bit for bit), then dH[3r + c] += d_r * c over the frame with
// c in (x, y, 1).  The per-sample values are exact to the bit; the SUM over the frame is a float
// sum whose order the reference fixes only by ATen's matmul blocking, so it is pinned by an
// error bound instead (tests/test_camgrad_gpu.py) -- but it is REPRODUCIBLE here: no float
// atomics, every partial sum has a fixed order that depends on the frame geometry alone, never on
// the plane groups, the workspace, the checkpoints or the stream:
//
//   bwd_cam_kernel      a block = 4 waves = a 64 x 8 output tile of one 8-plane chunk; lanes =
//                       (pixel, plane of the chunk) like the chain, so a tap instruction reads whole
//                       128-B pixel lines.  A lane adds its samples in (row, sub-step) order, the 8
//                       lanes of a plane are folded by xor shuffles, the 4 waves in LDS in wave order;
//                       one 9-float partial per (plane, tile).
//   bwd_cam_sum_kernel  a block per plane: thread t adds tiles t, t + 256, ... in double, a fixed
//                       LDS tree folds the 256 threads; one rounding to float at the end.
//
// A sample with no tap inside the image contributes exactly zero and its d sample is NOT read: the
// chain leaves the d samples of dead tiles unwritten (render_bwd.hip, round 6).  Tiles that
// tile_dead proves dead for a plane issue nothing for it.
#include "mpiv_common.hpp"

namespace mpiv {

constexpr int kCamTX = 64;   // tile width: 8 sub-steps of 8 pixels
constexpr int kCamRows = 2;  // rows per wave
constexpr int kCamTY = 4 * kCamRows;

// MODE 0: the reference's plain divisions (H or W < 2, as bwd_chain_kernel<0>); 1: the fast recipe
// with the per-sample division guard (the same bits as the chain's proven path wherever that runs).
// Chunk c_lo + blockIdx.y of the view (the grid's y spans the plane group whose d samples the window
// ws holds).
//
// The four divisions by the projective w share one refined reciprocal (mpiv_common.hpp div_core: the
// IEEE sequence without its range scaling, the correctly rounded quotient while operands and quotient
// stay in the normal range) and the two by H-1 and W-1 use div_const (Markstein, same condition) when
// every operand lies in [2^-60, 2^60] -- then all quotients lie in [2^-120, 2^120]; any other sample
// (a zero among them) takes the plain IEEE divisions.
__device__ __forceinline__ bool cam_mid(float a) {
    const float m = __builtin_fabsf(a);
    return m >= 0x1p-60f && m <= 0x1p60f;  // false for NaN
}

// TX: the texel type of the view (render_chunk.hip); a half tap's channels are converted (exactly) where
// the float kernel reads them, so the sums see the same values in the same order.
template <int MODE, bool WIDE, class TX = InF32>
__global__ __launch_bounds__(256) void bwd_cam_kernel(const typename TX::Scalar* __restrict__ view, RenderGeom g, ChunkGeom cg,
                                                      const float* __restrict__ homs, BwdWs ws, int c_lo,
                                                      float* __restrict__ partials, int ntiles) {
    constexpr int CH = kBwdCH;
    __shared__ float s_part[4][CH][9];
    const int tiles_x = (g.W + kCamTX - 1) / kCamTX;
    const int tile = blockIdx.x;
    const int tx0 = (tile % tiles_x) * kCamTX, ty0 = (tile / tiles_x) * kCamTY;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & (kWave - 1);
    const int j = lane % CH, i = lane / CH;
    const int64_t HW = (int64_t)g.H * g.W;
    const float rx0 = (float)tx0, rx1 = (float)min(tx0 + kCamTX - 1, g.W - 1);
    const float ry0 = (float)ty0, ry1 = (float)min(ty0 + kCamTY - 1, g.H - 1);
    {
        const int c = c_lo + (int)blockIdx.y;
        const int p = c * CH + j;
        float h[9];
        {
            const int pl = min(p, g.P - 1);
#pragma unroll
            for (int k = 0; k < 9; ++k) h[k] = homs[(int64_t)pl * 9 + k];
        }
        bool live = p < g.P;
        if (MODE != 0) live = live && !(div2_rect_safe(h, rx0, rx1, ry0, ry1) && tile_dead(h, rx0, rx1, ry0, ry1, g));
        float acc[9];
#pragma unroll
        for (int k = 0; k < 9; ++k) acc[k] = 0.0f;
        if (__any(live)) {
            for (int r = 0; r < kCamRows; ++r) {
                const int y = ty0 + wave * kCamRows + r;
                if (y >= g.H) break;  // wave-uniform
                const float fy = (float)y;
#pragma unroll 2
                for (int k = 0; k < kCamTX / 8; ++k) {
                    const int x = tx0 + k * 8 + i;
                    const float fx = (float)min(x, g.W - 1);
                    float px, py;
                    bwd_pos<MODE>(h, fx, fy, g, px, py);
                    ChunkTaps<TX> t;
                    int nt;
                    const bool on = live && x < g.W;
                    if constexpr (WIDE)
                        nt = issue_taps_chunk_wide<TX>(view + (int64_t)c * CH * 4, g, cg, j, on, px, py, t);
                    else
                        nt = issue_taps_chunk(make_rsrc(view + (int64_t)c * CH * 4, cg.rec_bytes), g, cg, j, on, px, py,
                                              t);
                    if (nt > 0) {  // (on: a lane that is off has no tap inside)
                        const float4 d4 = ds_plane(ws, p, HW)[(int64_t)y * g.W + x];
                        const float dsv[4] = {d4.x, d4.y, d4.z, d4.w};
                        const float w = t.wx, e = 1.0f - w, n = t.wy, s = 1.0f - n;
                        float gx = 0.0f, gy = 0.0f;
#pragma unroll
                        for (int q = 0; q < 4; ++q) {
                            const float ta = TX::chan(t.a, q), tb = TX::chan(t.b, q);
                            const float tc = TX::chan(t.c, q), td = TX::chan(t.d, q);
                            const float tx = __builtin_fmaf(td - tc, n, (tb - ta) * s);
                            gx = __builtin_fmaf(tx, dsv[q], gx);
                            const float ty = __builtin_fmaf(td - tb, w, (tc - ta) * e);
                            gy = __builtin_fmaf(ty, dsv[q], gy);
                        }
                        gx = gx * g.half_w;  // grid_sample's unnormalise multipliers
                        gy = gy * g.half_h;
                        const float gx2 = gx * 2.0f, gy2 = gy * 2.0f;
                        const float u = __builtin_fmaf(h[1], fy, h[0] * fx) + h[2];
                        const float v = __builtin_fmaf(h[4], fy, h[3] * fx) + h[5];
                        const float w3 = __builtin_fmaf(h[7], fy, h[6] * fx) + h[8];
                        const float wd = (w3 == 0.0f) ? w3 + 1e-8f : w3;  // divide_safe_torch, utils.py:38
                        float ax = 0.0f, ay = 0.0f, du = 0.0f, dv = 0.0f, quu = 0.0f, qvv = 0.0f;
                        bool fastdiv = false;
                        if (MODE != 0 && cam_mid(gx2) && cam_mid(gy2) && cam_mid(u) && cam_mid(v) && cam_mid(wd)) {
                            ax = div_const(gx2, g.hm1, g.rc_hm1);  // SWAPPED, utils.py:188 (H-1, W-1 in [1, 2^26))
                            ay = div_const(gy2, g.wm1, g.rc_wm1);
                            float yr = __builtin_amdgcn_rcpf(wd);
                            const float er = __builtin_fmaf(-wd, yr, 1.0f);
                            yr = __builtin_fmaf(er, yr, yr);
                            const float qu = div_core(u, wd, yr), qv = div_core(v, wd, yr);
                            if (cam_mid(ax) && cam_mid(ay) && cam_mid(qu) && cam_mid(qv)) {
                                fastdiv = true;
                                du = div_core(ax, wd, yr);
                                dv = div_core(ay, wd, yr);
                                quu = div_core(qu, wd, yr);
                                qvv = div_core(qv, wd, yr);
                            }
                        }
                        if (!fastdiv) {
                            ax = div_rn(gx2, g.hm1);
                            ay = div_rn(gy2, g.wm1);
                            du = div_rn(ax, wd);
                            dv = div_rn(ay, wd);
                            quu = div_rn(div_rn(u, wd), wd);
                            qvv = div_rn(div_rn(v, wd), wd);
                        }
                        const float dw = (-ax * quu) + (-ay * qvv);
                        acc[0] = acc[0] + du * fx;
                        acc[1] = acc[1] + du * fy;
                        acc[2] = acc[2] + du;
                        acc[3] = acc[3] + dv * fx;
                        acc[4] = acc[4] + dv * fy;
                        acc[5] = acc[5] + dv;
                        acc[6] = acc[6] + dw * fx;
                        acc[7] = acc[7] + dw * fy;
                        acc[8] = acc[8] + dw;
                    }
                }
            }
        }
        // the 8 lanes of a plane (lane bits 3..5); a + b is commutative, so every lane holds the same bits
#pragma unroll
        for (int k = 0; k < 9; ++k) {
            float a = acc[k];
            a = a + __shfl_xor(a, 8);
            a = a + __shfl_xor(a, 16);
            a = a + __shfl_xor(a, 32);
            acc[k] = a;
        }
        if (i == 0) {
#pragma unroll
            for (int k = 0; k < 9; ++k) s_part[wave][j][k] = acc[k];
        }
        __syncthreads();
        if (threadIdx.x < CH * 9) {
            const int jj = threadIdx.x / 9, k = threadIdx.x % 9;
            const int pp = c * CH + jj;
            if (pp < g.P) {
                float a = s_part[0][jj][k];
                a = a + s_part[1][jj][k];
                a = a + s_part[2][jj][k];
                a = a + s_part[3][jj][k];
                partials[((int64_t)pp * ntiles + tile) * 9 + k] = a;
            }
        }
    }
}

// dhoms[p][k] = sum over the tiles of partials[p][tile][k], in a fixed order, accumulated in double
__global__ __launch_bounds__(256) void bwd_cam_sum_kernel(const float* __restrict__ partials, int ntiles,
                                                          float* __restrict__ dhoms) {
    __shared__ double s_sum[256][9];
    const int p = blockIdx.x, t = threadIdx.x;
    double a[9];
#pragma unroll
    for (int k = 0; k < 9; ++k) a[k] = 0.0;
    for (int tile = t; tile < ntiles; tile += 256) {
        const float* q = partials + ((int64_t)p * ntiles + tile) * 9;
#pragma unroll
        for (int k = 0; k < 9; ++k) a[k] = a[k] + (double)q[k];
    }
#pragma unroll
    for (int k = 0; k < 9; ++k) s_sum[t][k] = a[k];
    __syncthreads();
    for (int off = 128; off >= 1; off >>= 1) {
        if (t < off) {
#pragma unroll
            for (int k = 0; k < 9; ++k) s_sum[t][k] = s_sum[t][k] + s_sum[t + off][k];
        }
        __syncthreads();
    }
    if (t < 9) dhoms[(int64_t)p * 9 + t] = (float)s_sum[0][t];
}

}  // namespace mpiv
