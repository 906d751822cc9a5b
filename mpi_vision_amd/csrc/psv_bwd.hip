// psv_bwd.hip -- the adjoint of the plane sweep (autograd of plane_sweep_torch, utils.py:452-471, and of
// its _one / _one2 forms and format_network_input_torch's volumes) w.r.t. the source image, the plane
// depths and the two camera matrices Ki = inverse(K_tgt) and proj = K4_src @ pose.
//
// The reference's sweep is D inverse warps on constant depth maps and a torch.cat on the channel axis, so
// the volume's adjoint is D of warp_bwd.hip's adjoints over one source, depth d reading the channels
// d*C .. d*C+C-1 of dout.  The (view, depth) pairs of a plane group are the views of warp_bwd.hip's
// batched sort; what this file adds is
//
// (a) psv_bwd_pixel_kernel: one work-item per target pixel, the ray computed once, then per depth of the
//     group warp_bwd_pixel_kernel's body line for line on the constant depth: the sample position and
//     bucket key of (view, depth), and the block's sums of 22 per-pixel products, the 21 of dki / dproj
//     and the per-pixel d depth, (dcam_0 * rx + dcam_1 * ry) + dcam_2 * rz.
//
// (b) psv_bwd_cam_sum_kernel / psv_bwd_depth_sum_kernel: dki[b], dproj[b] = the sum over all depths and
//     blocks, ddepths[d] = the sum over all views and blocks, of the blocks' partials, each accumulated in
//     double in a fixed order and rounded once.  The partials of every depth are kept (they are not part
//     of a group's share of the workspace), so the sums do not depend on the grouping.
//
// (c) psv_bwd_bounds_kernel: after the sort, start[bucket] and end[bucket] of every (view, depth) wherever
//     adjacent sorted keys differ, into a table cleared before (an empty bucket reads start == end): the
//     gather finds a texel's four buckets with four reads instead of eight binary searches per plane.
//
// (d) psv_bwd_gather_kernel: one work-item per source texel.  For d from the group's highest plane down
//     to its lowest, g_d is accumulated from +0 in warp_bwd_gather_kernel's merge order (8-pixel chunk,
//     then corner nw / ne / sw / se, then ascending pixel) and added to the texel's accumulator:
//     ((g_{D-1} + g_{D-2}) + ...) + g_0, the order in which autograd adds the D grid_sample gradients
//     into the leaf (the consumer created last runs first).  The first plane of the first group is the
//     accumulator; later groups read dimg back, so the bits do not depend on the group size.
//
// Every loop is bounded by counts clamped to the pixel count; no kernel waits on another block; no float
// atomics.
#include "mpiv_common.hpp"

namespace mpiv {

constexpr int kPsvCam = kWarpCam + 1;  // the 21 camera products and the per-pixel d depth

// arrays of the workspace (mpiv_plane_sweep_backward_workspace_size): those of WarpBwdWs for the B*G
// (view, depth) pairs of one plane group, the bucket bounds table, and the partials of all D depths
struct PsvBwdWs {
    float2* pos;       // [B*G][N] sample positions
    unsigned* key[2];  // [B*G][N] bucket ids (ping-pong)
    unsigned* id[2];   // [B*G][N] pixel ids (ping-pong)
    unsigned* hist;    // [B*G][256][nblk]
    unsigned* totals;  // [B*G][256]
    uint2* table;      // [B*G][(Hs+1)*(Ws+1)] (start, end) of each bucket in the sorted ids
    float* partials;   // [B][D][nblk][kPsvCam]
};

// planes d0 .. d0+G-1 of a group; (view b, plane d0+g) is pair b*G+g of pos / key
__global__ __launch_bounds__(kWarpThreads) void psv_bwd_pixel_kernel(
    const float* __restrict__ img, ImgStrides s, SweepParams sp, const float* __restrict__ ki,
    const float* __restrict__ proj, const float* __restrict__ depths, int d0, int G,
    const float* __restrict__ dout, ImgStrides ds, float2* __restrict__ pos, unsigned* __restrict__ key,
    float* __restrict__ partials, unsigned nblk) {
    __shared__ float s_part[kWarpThreads / kWave][kPsvCam];
    const unsigned npix = (unsigned)sp.Ht * (unsigned)sp.Wt;  // < 2^31, checked on the host
    const unsigned gid = blockIdx.x * kWarpThreads + threadIdx.x;
    const int b = blockIdx.y;
    const bool on = gid < npix;
    const unsigned pix = on ? gid : npix - 1;  // tail lanes recompute the last pixel and contribute +0
    const int y = (int)(pix / (unsigned)sp.Wt), x = (int)(pix % (unsigned)sp.Wt);
    const float fx = (float)x, fy = (float)y;
    const float* m = proj + (int64_t)b * 16;
    float rx, ry, rz;
    ray(ki + (int64_t)b * 9, fx, fy, rx, ry, rz);
    const unsigned nb = (unsigned)(sp.Hs + 1) * (unsigned)(sp.Ws + 1);
    const float* src = img + (int64_t)b * s.b;
    const float* dq0 = dout + b * ds.b + y * ds.y + x * ds.x;
    const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x >> 6;
    for (int g = 0; g < G; ++g) {  // (uniform trip count)
        const int d = d0 + g;
        const float dep = depths[d];
        // sweep_pos, with its intermediates kept
        const float X = rx * dep, Y = ry * dep, Z = rz * dep;
        const float pu = __builtin_fmaf(m[2], Z, __builtin_fmaf(m[1], Y, m[0] * X)) + m[3];
        const float pv = __builtin_fmaf(m[6], Z, __builtin_fmaf(m[5], Y, m[4] * X)) + m[7];
        const float pz = __builtin_fmaf(m[10], Z, __builtin_fmaf(m[9], Y, m[8] * X)) + m[11];
        const float den = pz + 1e-10f;
        const float qu = div_rn(pu, den), qv = div_rn(pv, den);
        const float cx = div_rn(qu + 0.5f, sp.fhs);  // SWAPPED: x / H
        const float cy = div_rn(qv + 0.5f, sp.fws);  //          y / W
        const float px = unnormalize(to_grid(cx), sp.half_ws);
        const float py = unnormalize(to_grid(cy), sp.half_hs);
        const Bilinear bl = bilinear_setup(px, py, sp.Ws, sp.Hs);
        const bool m00 = bl.x0 & bl.y0, m10 = bl.x1 & bl.y0, m01 = bl.x0 & bl.y1, m11 = bl.x1 & bl.y1;
        if (on && pos != nullptr) {
            const bool has = (bl.x0 | bl.x1) & (bl.y0 | bl.y1);  // a corner inside the image (false for NaN)
            const int64_t at = ((int64_t)b * G + g) * npix + pix;
            pos[at] = make_float2(px, py);
            key[at] = has ? (unsigned)(bl.iy + 1) * (unsigned)(sp.Ws + 1) + (unsigned)(bl.ix + 1) : nb;
        }
        if (partials == nullptr) continue;  // (uniform: only d img was asked for)

        const float fx0 = floorf(px), fy0 = floorf(py);
        const float w = px - fx0, e = 1.0f - w, n = py - fy0, sth = 1.0f - n;
        const float* dq = dq0 + (int64_t)d * sp.C * ds.c;
        float gx = 0.0f, gy = 0.0f;
        for (int c = 0; c < sp.C; ++c) {
            const float ta = ld_img(src, s, bl.ix, bl.iy, c, m00), tb = ld_img(src, s, bl.ix + 1, bl.iy, c, m10);
            const float tc = ld_img(src, s, bl.ix, bl.iy + 1, c, m01), td = ld_img(src, s, bl.ix + 1, bl.iy + 1, c, m11);
            const float dc = dq[c * ds.c];
            const float tx = __builtin_fmaf(td - tc, n, (tb - ta) * sth);
            gx = __builtin_fmaf(tx, dc, gx);
            const float ty = __builtin_fmaf(td - tb, w, (tc - ta) * e);
            gy = __builtin_fmaf(ty, dc, gy);
        }
        gx = gx * sp.half_ws;  // grid_sample's unnormalise multipliers
        gy = gy * sp.half_hs;
        const float ax = div_rn(gx * 2.0f, sp.fhs);  // SWAPPED, as the forward
        const float ay = div_rn(gy * 2.0f, sp.fws);
        const float du = div_rn(ax, den) + 0.0f;
        const float dv = div_rn(ay, den) + 0.0f;
        const float dz = ((-ax * div_rn(qu, den)) + (-ay * div_rn(qv, den))) + 0.0f;
        float dcam[3];
#pragma unroll
        for (int k = 0; k < 3; ++k)
            dcam[k] = __builtin_fmaf(m[8 + k], dz, __builtin_fmaf(m[4 + k], dv, m[k] * du)) + 0.0f;
        const float ddep = (dcam[0] * rx + dcam[1] * ry) + dcam[2] * rz;

        float v[kPsvCam];
        {
            const float pc[3] = {fx, fy, 1.0f}, cam[4] = {X, Y, Z, 1.0f}, d3[3] = {du, dv, dz};
#pragma unroll
            for (int i = 0; i < 3; ++i) {
                const float dr = dcam[i] * dep;  // d (Ki @ pixels)_i
#pragma unroll
                for (int j = 0; j < 3; ++j) v[3 * i + j] = on ? dr * pc[j] : 0.0f;
#pragma unroll
                for (int k = 0; k < 4; ++k) v[9 + 4 * i + k] = on ? d3[i] * cam[k] : 0.0f;
            }
            v[kWarpCam] = on ? ddep : 0.0f;
        }
#pragma unroll
        for (int k = 0; k < kPsvCam; ++k) {  // a + b is commutative: every lane holds the same bits
            float a = v[k];
#pragma unroll
            for (int o = 1; o < kWave; o <<= 1) a = a + __shfl_xor(a, o);
            if (lane == 0) s_part[wave][k] = a;
        }
        __syncthreads();
        if (threadIdx.x < kPsvCam) {
            const int k = threadIdx.x;
            float a = s_part[0][k];
            a = a + s_part[1][k];
            a = a + s_part[2][k];
            a = a + s_part[3][k];
            partials[(((int64_t)b * sp.D + d) * nblk + blockIdx.x) * kPsvCam + k] = a;
        }
        __syncthreads();  // s_part is rewritten for the next depth
    }
}

// dki[b][0..8], dproj[b][0..15] = the sum over the depths and blocks of partials[b][d][blk][k], in double
// in a fixed order, one rounding at the end; dproj's row 3 is +0 (warp_bwd_cam_sum_kernel's scheme)
__global__ __launch_bounds__(256) void psv_bwd_cam_sum_kernel(const float* __restrict__ partials, unsigned nblk, int D,
                                                              float* __restrict__ dki, float* __restrict__ dproj) {
    __shared__ double s_sum[256][kWarpCam];
    const int b = blockIdx.x, t = threadIdx.x;
    const int64_t cnt = (int64_t)D * nblk;  // view b's records are contiguous: [d][blk]
    double a[kWarpCam];
#pragma unroll
    for (int k = 0; k < kWarpCam; ++k) a[k] = 0.0;
    for (int64_t r = t; r < cnt; r += 256) {
        const float* q = partials + ((int64_t)b * cnt + r) * kPsvCam;
#pragma unroll
        for (int k = 0; k < kWarpCam; ++k) a[k] = a[k] + (double)q[k];
    }
#pragma unroll
    for (int k = 0; k < kWarpCam; ++k) s_sum[t][k] = a[k];
    __syncthreads();
    for (int off = 128; off >= 1; off >>= 1) {
        if (t < off) {
#pragma unroll
            for (int k = 0; k < kWarpCam; ++k) s_sum[t][k] = s_sum[t][k] + s_sum[t + off][k];
        }
        __syncthreads();
    }
    if (t < 9 && dki != nullptr) dki[(int64_t)b * 9 + t] = (float)s_sum[0][t];
    if (t < 16 && dproj != nullptr) dproj[(int64_t)b * 16 + t] = t < 12 ? (float)s_sum[0][9 + t] : 0.0f;
}

// ddepths[d] = the sum over the views and blocks of partials[b][d][blk][21], the same way
__global__ __launch_bounds__(256) void psv_bwd_depth_sum_kernel(const float* __restrict__ partials, unsigned nblk, int B,
                                                                int D, float* __restrict__ ddepths) {
    __shared__ double s_sum[256];
    const int d = blockIdx.x, t = threadIdx.x;
    double a = 0.0;
    for (int b = 0; b < B; ++b) {
        const float* q = partials + (((int64_t)b * D + d) * nblk) * kPsvCam + kWarpCam;
        for (unsigned blk = t; blk < nblk; blk += 256) a = a + (double)q[(int64_t)blk * kPsvCam];
    }
    s_sum[t] = a;
    __syncthreads();
    for (int off = 128; off >= 1; off >>= 1) {
        if (t < off) s_sum[t] = s_sum[t] + s_sum[t + off];
        __syncthreads();
    }
    if (t == 0) ddepths[d] = (float)s_sum[0];
}

__global__ __launch_bounds__(256) void psv_bwd_clear_kernel(uint2* __restrict__ table, unsigned nb) {
    const unsigned i = blockIdx.x * 256 + threadIdx.x;
    if (i < nb) table[(int64_t)blockIdx.y * nb + i] = make_uint2(0u, 0u);
}

// table[pair][k] = (first index, one past the last index) of key k in the pair's sorted keys, k < nb
__global__ __launch_bounds__(256) void psv_bwd_bounds_kernel(const unsigned* __restrict__ keys, unsigned n, unsigned nb,
                                                             uint2* __restrict__ table) {
    const unsigned i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const unsigned* kv = keys + (int64_t)blockIdx.y * n;
    const unsigned k = kv[i];
    if (k >= nb) return;  // the "no bucket" key
    uint2* e = table + (int64_t)blockIdx.y * nb + k;
    if (i == 0 || kv[i - 1] != k) e->x = i;
    if (i == n - 1 || kv[i + 1] != k) e->y = i + 1;
}

// one work-item per source texel, planes d0+G-1 down to d0 (see (d) above); `first`: no plane has been
// added to dimg yet
__global__ __launch_bounds__(256) void psv_bwd_gather_kernel(const unsigned* __restrict__ ids,
                                                             const float2* __restrict__ pos,
                                                             const uint2* __restrict__ table,
                                                             const float* __restrict__ dout, ImgStrides ds,
                                                             SweepParams sp, FastDiv fd_wt, int d0, int G, int first,
                                                             float* __restrict__ dimg) {
    const unsigned ntex = (unsigned)sp.Hs * (unsigned)sp.Ws, n = (unsigned)sp.Ht * (unsigned)sp.Wt;
    const unsigned tex = blockIdx.x * 256 + threadIdx.x;
    const int b = blockIdx.y;
    if (tex >= ntex) return;
    const unsigned ty = tex / (unsigned)sp.Ws, tx = tex - ty * (unsigned)sp.Ws;
    const unsigned bw = (unsigned)sp.Ws + 1, nb = (unsigned)(sp.Hs + 1) * bw;
    // corner k of a pixel whose nw tap is (ix, iy) = (tx - (k & 1), ty - (k >> 1)): bucket (ix + 1, iy + 1)
    unsigned bk[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) bk[k] = (ty + 1 - (k >> 1)) * bw + (tx + 1 - (k & 1));  // < nb
    float* o = dimg + ((int64_t)b * ntex + tex) * sp.C;
    for (int c0 = 0; c0 < sp.C; c0 += 4) {
        const int nc = min(4, sp.C - c0);
        float acc[4] = {0.0f, 0.0f, 0.0f, 0.0f};
        bool have = first == 0;
        if (have) {
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (j < nc) acc[j] = o[c0 + j];
        }
        for (int g = G - 1; g >= 0; --g) {
            const int64_t pair = (int64_t)b * G + g;
            const unsigned* idv = ids + pair * n;
            const float2* posv = pos + pair * n;
            const uint2* tb = table + pair * nb;
            const float* dq = dout + b * ds.b + ((int64_t)(d0 + g) * sp.C + c0) * ds.c;
            unsigned p[4], hi[4], total = 0;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const uint2 e = tb[bk[k]];
                hi[k] = min(e.y, n);
                p[k] = min(e.x, hi[k]);
                total += hi[k] - p[k];
            }
            total = min(total, n);  // (a pixel has one bucket: the four counts sum to at most n)
            float gd[4] = {0.0f, 0.0f, 0.0f, 0.0f};
            unsigned done = 0;
            while (done < total) {
                unsigned cur = 0xFFFFFFFFu;  // the lowest 8-pixel chunk among the four heads
#pragma unroll
                for (int k = 0; k < 4; ++k)
                    if (p[k] < hi[k]) cur = min(cur, min(idv[p[k]], n - 1) >> 3);
                if (cur == 0xFFFFFFFFu) break;
                unsigned step = 0;
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    while (p[k] < hi[k]) {
                        const unsigned id = min(idv[p[k]], n - 1);
                        if ((id >> 3) != cur) break;
                        const float2 q = posv[id];
                        const Bilinear bl = bilinear_setup(q.x, q.y, sp.Ws, sp.Hs);
                        const float wk = k == 0 ? bl.nw : k == 1 ? bl.ne : k == 2 ? bl.sw : bl.se;
                        const unsigned yy = fast_div(id, fd_wt), xx = id - yy * (unsigned)sp.Wt;
                        const float* dd = dq + yy * ds.y + xx * ds.x;
#pragma unroll
                        for (int j = 0; j < 4; ++j)
                            if (j < nc) gd[j] = gd[j] + wk * dd[j * ds.c];
                        ++p[k];
                        ++step;
                    }
                }
                if (step == 0) break;  // (never: the head that set `cur` is consumed)
                done += step;
            }
#pragma unroll
            for (int j = 0; j < 4; ++j) acc[j] = have ? acc[j] + gd[j] : gd[j];
            have = true;
        }
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (j < nc) o[c0 + j] = acc[j];
    }
}

}  // namespace mpiv
