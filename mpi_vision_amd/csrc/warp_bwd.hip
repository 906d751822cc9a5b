// warp_bwd.hip -- the adjoint of the depth-map inverse warp (autograd of
// projective_inverse_warp_torch[2], utils.py:409-450, 725-769) w.r.t. the depth map, the source
// image and the two camera matrices Ki = inverse(K_tgt) and proj = K4_src @ pose (the chain from
// there to pose and intrinsics is a handful of numbers and stays in torch on the host,
// _host.psv_matrices_autograd).
//
// (a) warp_bwd_pixel_kernel: one work-item per target pixel.  The forward's position is recomputed
//     with the forward's own operations (ray / the body of sweep_pos / bilinear_setup: the tap set
//     depends on its bits), then
//
//       gx = gy = +0;  per c:  tx = fma(se_c - sw_c, n, (ne_c - nw_c) * s);  gx = fma(tx, dout_c, gx)
//                              ty = fma(se_c - ne_c, w, (sw_c - nw_c) * e);  gy = fma(ty, dout_c, gy)
//       gx *= Ws/2;  gy *= Hs/2;  ax = (gx * 2) / Hs;  ay = (gy * 2) / Ws     (swapped, no -1 here)
//       den = pz + 1e-10f;  du = ax / den + 0;  dv = ay / den + 0
//       dz = ((-ax * ((pu / den) / den)) + (-ay * ((pv / den) / den))) + 0
//       dcam_k = fma(proj[2][k], dz, fma(proj[1][k], dv, proj[0][k] * du)) + 0          (k = 0..2)
//       ddepth = (dcam_0 * rx + dcam_1 * ry) + dcam_2 * rz
//       dproj[r][k] += d_r * cam_k  (cam = (X, Y, Z, 1));   dki[i][j] += (dcam_i * depth) * (x, y, 1)_j
//
//     every line one fp32 rounding, the divisions IEEE, no divide-safe (the reference has none: its
//     Inf / NaN pattern is reproduced).  The `+ 0` are autograd's sums of the two slice gradients of
//     proj @ cam (rows 0..1 and row 2, each padded with zeros) and the zero fourth term of MKL's
//     backward sgemm: they turn a -0 into +0.  dcam_k is that sgemm's FMA chain in ascending row order,
//     the pattern of the forward's ray / sweep_pos; ddepth is ATen's sum_to_size, plain adds in
//     ascending order.  Both were pinned against the reference's tapped gradients
//     (tools/gen_goldens_warpgrad.py): each is the only one of the 12 candidates (6 orders, fused or
//     not) that matches every pixel of every golden case.
//
// (b) dki / dproj: a block adds its 256 pixels' products in a fixed order (xor shuffles within a wave,
//     the 4 waves in wave order), warp_bwd_cam_sum_kernel adds the blocks' partials in double in a
//     fixed order and rounds once: no float atomics, the same bits whatever else was requested
//     (render_bwd_cam.hip's scheme).
//
// (c) dimg: per texel, the contributions w_corner * dout_c (one rounding each) are added from +0 in
//     ATen's CPU order: ascending 8-pixel chunk of the flat target index, within a chunk the corners
//     nw, ne, sw, se, within a corner ascending pixel.  A depth map is an arbitrary coordinate field, so
//     the contributors of a texel are found by sorting: a pixel's bucket is its nw tap (ix+1, iy+1) in
//     an (Hs+1) x (Ws+1) grid (none when no corner lies inside the image); the pixel ids are sorted by
//     bucket with a stable LSD radix sort (per pass: per-block digit histograms, a scan per digit, an in-block
//     stable rank by wave ballots), which leaves each bucket's pixels ascending; then one work-item per
//     texel merges the four buckets in which it is the nw, ne, sw and se corner.  Every loop is bounded
//     by counts clamped to the pixel count; no kernel waits on another block.
#include "mpiv_common.hpp"

namespace mpiv {

constexpr int kWarpCam = 21;       // per-pixel products summed over the frame: 9 of dki, 12 of dproj rows 0..2
constexpr int kWarpThreads = 256;  // pixels per block of the pixel pass and of a sort tile

// per-view arrays of the workspace (mpiv_inverse_warp_backward_workspace_size)
struct WarpBwdWs {
    float2* pos;         // [B][N] sample positions
    unsigned* key[2];    // [B][N] bucket ids (ping-pong)
    unsigned* id[2];     // [B][N] pixel ids (ping-pong)
    unsigned* hist;      // [B][256][nblk] digit histograms -> offsets within the digit
    unsigned* totals;    // [B][256] keys per digit
    float* partials;     // [B][nblk][kWarpCam]
};

__global__ __launch_bounds__(kWarpThreads) void warp_bwd_pixel_kernel(
    const float* __restrict__ img, ImgStrides s, SweepParams sp, const float* __restrict__ ki,
    const float* __restrict__ proj, const float* __restrict__ depth, int64_t dsb, int64_t dsy, int64_t dsx,
    const float* __restrict__ dout, ImgStrides ds, float* __restrict__ ddepth, float2* __restrict__ pos,
    unsigned* __restrict__ key, float* __restrict__ partials, unsigned nblk) {
    __shared__ float s_part[kWarpThreads / kWave][kWarpCam];
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
    const float dep = depth[b * dsb + y * dsy + x * dsx];
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
        const unsigned nb = (unsigned)(sp.Hs + 1) * (unsigned)(sp.Ws + 1);
        pos[(int64_t)b * npix + pix] = make_float2(px, py);
        key[(int64_t)b * npix + pix] = has ? (unsigned)(bl.iy + 1) * (unsigned)(sp.Ws + 1) + (unsigned)(bl.ix + 1) : nb;
    }
    if (ddepth == nullptr && partials == nullptr) return;  // (uniform: only d img was asked for)

    const float fx0 = floorf(px), fy0 = floorf(py);
    const float w = px - fx0, e = 1.0f - w, n = py - fy0, sth = 1.0f - n;
    const float* src = img + (int64_t)b * s.b;
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
    const float ax = div_rn(gx * 2.0f, sp.fhs);  // SWAPPED, as the forward
    const float ay = div_rn(gy * 2.0f, sp.fws);
    const float du = div_rn(ax, den) + 0.0f;
    const float dv = div_rn(ay, den) + 0.0f;
    const float dz = ((-ax * div_rn(qu, den)) + (-ay * div_rn(qv, den))) + 0.0f;
    float dcam[3];
#pragma unroll
    for (int k = 0; k < 3; ++k)
        dcam[k] = __builtin_fmaf(m[8 + k], dz, __builtin_fmaf(m[4 + k], dv, m[k] * du)) + 0.0f;
    if (on && ddepth != nullptr) ddepth[(int64_t)b * npix + pix] = (dcam[0] * rx + dcam[1] * ry) + dcam[2] * rz;
    if (partials == nullptr) return;  // (uniform)

    float v[kWarpCam];
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
    }
    const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x >> 6;
#pragma unroll
    for (int k = 0; k < kWarpCam; ++k) {  // a + b is commutative: every lane holds the same bits
        float a = v[k];
#pragma unroll
        for (int o = 1; o < kWave; o <<= 1) a = a + __shfl_xor(a, o);
        if (lane == 0) s_part[wave][k] = a;
    }
    __syncthreads();
    if (threadIdx.x < kWarpCam) {
        const int k = threadIdx.x;
        float a = s_part[0][k];
        a = a + s_part[1][k];
        a = a + s_part[2][k];
        a = a + s_part[3][k];
        partials[((int64_t)b * nblk + blockIdx.x) * kWarpCam + k] = a;
    }
}

// dki[b][0..8], dproj[b][0..15] = the sum over the blocks of partials[b][blk][k], accumulated in
// double in a fixed order, one rounding at the end; dproj's row 3 is +0 (its gradient is zero: the
// projective division reads rows 0..2 only)
__global__ __launch_bounds__(256) void warp_bwd_cam_sum_kernel(const float* __restrict__ partials, unsigned nblk,
                                                               float* __restrict__ dki, float* __restrict__ dproj) {
    __shared__ double s_sum[256][kWarpCam];
    const int b = blockIdx.x, t = threadIdx.x;
    double a[kWarpCam];
#pragma unroll
    for (int k = 0; k < kWarpCam; ++k) a[k] = 0.0;
    for (unsigned blk = t; blk < nblk; blk += 256) {
        const float* q = partials + ((int64_t)b * nblk + blk) * kWarpCam;
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

// ---- stable LSD radix sort of the pixel ids by bucket, 8 bits per pass, 256 elements per block ----

// hist[b][digit][blk] = how many of block blk's keys have that digit
__global__ __launch_bounds__(kWarpThreads) void warp_sort_hist_kernel(const unsigned* __restrict__ key_in, unsigned n,
                                                                      unsigned nblk, int shift,
                                                                      unsigned* __restrict__ hist) {
    __shared__ unsigned s_h[256];
    const unsigned t = threadIdx.x, i = blockIdx.x * kWarpThreads + t;
    const int b = blockIdx.y;
    s_h[t] = 0;
    __syncthreads();
    if (i < n) atomicAdd(&s_h[(key_in[(int64_t)b * n + i] >> shift) & 255u], 1u);  // (integer counts: any order)
    __syncthreads();
    hist[((int64_t)b * 256 + t) * nblk + blockIdx.x] = s_h[t];
}

// block (digit, view): in place, the exclusive prefix sum of hist[b][digit][0..nblk) over the blocks, and
// the digit's total into totals[b][digit] (the scatter adds the totals of the lower digits)
__global__ __launch_bounds__(256) void warp_sort_scan_kernel(unsigned* __restrict__ hist, unsigned nblk,
                                                             unsigned* __restrict__ totals) {
    __shared__ unsigned s_s[256];
    const unsigned t = threadIdx.x;
    unsigned* h = hist + ((int64_t)blockIdx.y * 256 + blockIdx.x) * nblk;
    unsigned carry = 0;
    for (unsigned i0 = 0; i0 < nblk; i0 += 256) {  // (block-uniform trip count)
        const unsigned v = i0 + t < nblk ? h[i0 + t] : 0u;
        s_s[t] = v;
        __syncthreads();
        for (unsigned off = 1; off < 256; off <<= 1) {  // inclusive scan of the chunk
            const unsigned u = t >= off ? s_s[t - off] : 0u;
            __syncthreads();
            s_s[t] += u;
            __syncthreads();
        }
        if (i0 + t < nblk) h[i0 + t] = carry + s_s[t] - v;
        carry += s_s[255];
        __syncthreads();
    }
    if (t == 0) totals[(int64_t)blockIdx.y * 256 + blockIdx.x] = carry;
}

// element i of block blk goes to offset[digit][blk] + (elements of the block with the same digit before
// it): the rank within a wave from ballots over the digit's bits, the waves before it from LDS counts
__global__ __launch_bounds__(kWarpThreads) void warp_sort_scatter_kernel(
    const unsigned* __restrict__ key_in, const unsigned* __restrict__ id_in, unsigned* __restrict__ key_out,
    unsigned* __restrict__ id_out, const unsigned* __restrict__ hist, const unsigned* __restrict__ totals, unsigned n,
    unsigned nblk, int shift) {
    __shared__ unsigned s_cnt[kWarpThreads / kWave][256];
    __shared__ unsigned s_base[256];  // keys of this view with a lower digit
    const unsigned t = threadIdx.x, i = blockIdx.x * kWarpThreads + t;
    const int b = blockIdx.y;
    const unsigned lane = t & (kWave - 1), wave = t >> 6;
#pragma unroll
    for (int k = 0; k < kWarpThreads / kWave; ++k) s_cnt[k][t] = 0;
    const unsigned tot = totals[(int64_t)b * 256 + t];
    s_base[t] = tot;
    __syncthreads();
    for (unsigned off = 1; off < 256; off <<= 1) {  // inclusive scan of the 256 digit totals
        const unsigned u = t >= off ? s_base[t - off] : 0u;
        __syncthreads();
        s_base[t] += u;
        __syncthreads();
    }
    const unsigned mine = s_base[t] - tot;
    __syncthreads();
    s_base[t] = mine;
    __syncthreads();
    const bool valid = i < n;
    const unsigned k = valid ? key_in[(int64_t)b * n + i] : 0u;
    const unsigned d = (k >> shift) & 255u;
    unsigned long long peers = __ballot(valid);
#pragma unroll
    for (int bit = 0; bit < 8; ++bit) {
        const bool set = (d >> bit) & 1u;
        const unsigned long long bb = __ballot(set);
        peers &= set ? bb : ~bb;
    }
    const unsigned rank = (unsigned)__popcll(peers & ((1ull << lane) - 1ull));
    if (valid && rank == 0) s_cnt[wave][d] = (unsigned)__popcll(peers);
    __syncthreads();
    if (valid) {
        unsigned off = 0;
        for (unsigned w = 0; w < wave; ++w) off += s_cnt[w][d];
        const unsigned dst = s_base[d] + hist[((int64_t)b * 256 + d) * nblk + blockIdx.x] + off + rank;
        if (dst < n) {  // (always: the offsets are a permutation of [0, n))
            key_out[(int64_t)b * n + dst] = k;
            id_out[(int64_t)b * n + dst] = id_in != nullptr ? id_in[(int64_t)b * n + i] : i;
        }
    }
}

// first index in the sorted keys [0, n) whose key is >= k
__device__ __forceinline__ unsigned warp_lower_bound(const unsigned* __restrict__ keys, unsigned n, unsigned k) {
    unsigned lo = 0, hi = n;
    for (int it = 0; it < 32 && lo < hi; ++it) {
        const unsigned mid = lo + ((hi - lo) >> 1);
        if (keys[mid] < k) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

// one work-item per source texel: its contributors from the four buckets in which it is the nw, ne, sw
// and se corner, merged by ascending 8-pixel chunk, within a chunk by corner, within a corner by pixel
__global__ __launch_bounds__(256) void warp_bwd_gather_kernel(const unsigned* __restrict__ keys,
                                                              const unsigned* __restrict__ ids,
                                                              const float2* __restrict__ pos,
                                                              const float* __restrict__ dout, ImgStrides ds,
                                                              SweepParams sp, FastDiv fd_wt, float* __restrict__ dimg) {
    const unsigned ntex = (unsigned)sp.Hs * (unsigned)sp.Ws, n = (unsigned)sp.Ht * (unsigned)sp.Wt;
    const unsigned tex = blockIdx.x * 256 + threadIdx.x;
    const int b = blockIdx.y;
    if (tex >= ntex) return;
    const unsigned ty = tex / (unsigned)sp.Ws, tx = tex - ty * (unsigned)sp.Ws;
    const unsigned bw = (unsigned)sp.Ws + 1;
    keys += (int64_t)b * n;
    ids += (int64_t)b * n;
    pos += (int64_t)b * n;
    const float* dq = dout + b * ds.b;
    // corner k of a pixel whose nw tap is (ix, iy) = (tx - (k & 1), ty - (k >> 1)): bucket (ix + 1, iy + 1)
    unsigned lo[4], hi[4], total = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const unsigned bk = (ty + 1 - (k >> 1)) * bw + (tx + 1 - (k & 1));
        lo[k] = warp_lower_bound(keys, n, bk);
        hi[k] = warp_lower_bound(keys, n, bk + 1);
        total += hi[k] - lo[k];
    }
    total = min(total, n);  // (a pixel has one bucket: the four counts sum to at most n)
    float* o = dimg + ((int64_t)b * ntex + tex) * sp.C;
    for (int c0 = 0; c0 < sp.C; c0 += 4) {
        const int nc = min(4, sp.C - c0);
        float acc[4] = {0.0f, 0.0f, 0.0f, 0.0f};
        unsigned p[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) p[k] = lo[k];
        unsigned done = 0;
        while (done < total) {
            unsigned cur = 0xFFFFFFFFu;  // the lowest 8-pixel chunk among the four heads
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if (p[k] < hi[k]) cur = min(cur, min(ids[p[k]], n - 1) >> 3);
            if (cur == 0xFFFFFFFFu) break;
            unsigned step = 0;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                while (p[k] < hi[k]) {
                    const unsigned id = min(ids[p[k]], n - 1);
                    if ((id >> 3) != cur) break;
                    const float2 q = pos[id];
                    const Bilinear bl = bilinear_setup(q.x, q.y, sp.Ws, sp.Hs);
                    const float wk = k == 0 ? bl.nw : k == 1 ? bl.ne : k == 2 ? bl.sw : bl.se;
                    const unsigned yy = fast_div(id, fd_wt), xx = id - yy * (unsigned)sp.Wt;
                    const float* d = dq + yy * ds.y + xx * ds.x + c0 * ds.c;
#pragma unroll
                    for (int j = 0; j < 4; ++j)
                        if (j < nc) acc[j] = acc[j] + wk * d[j * ds.c];
                    ++p[k];
                    ++step;
                }
            }
            if (step == 0) break;  // (never: the head that set `cur` is consumed)
            done += step;
        }
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (j < nc) o[c0 + j] = acc[j];
    }
}

}  // namespace mpiv
