// render_kernels.inc -- the two sampling kernels of render.hip, included twice by it:
//   MPIV_GEOM = RenderGeom,  MPIV_KERNEL(name) = name##_kernel      the same-size render
//   MPIV_GEOM = RenderGeomT, MPIV_KERNEL(name) = name##_tgt_kernel  a target frame of its own size
// Everything that follows the target grid -- the tiling, the x / y bounds, the output index --
// reads tgt_w(g) / tgt_h(g); everything on the sample path takes g as a RenderGeom (the source).
// The contracts are documented in render.hip, above the include.

template <bool CT, bool FAST>
__global__ __launch_bounds__(256) void MPIV_KERNEL(render_packed)(const float4* __restrict__ planes,
                                                            int64_t plane_stride, MPIV_GEOM g, int V,
                                                            int p_begin, int p_end, int back,
                                                            const float* __restrict__ homs,
                                                            float* __restrict__ out, int order = 0) {
    const int tiles_x = (tgt_w(g) + kTileX - 1) / kTileX;
    const int lb = xcd_logical_block(blockIdx.x, gridDim.x);
    const int v = lb % V;
    const int tile = xcd_tile_order(lb / V, (int)gridDim.x / V, tiles_x, order);
    const int tx0 = (tile % tiles_x) * kTileX, ty0 = (tile / tiles_x) * kTileY;
    const int x = tx0 + (threadIdx.x & (kWave - 1));
    const int y = ty0 + (threadIdx.x >> 6);
    const float* hv = homs + (int64_t)v * g.P * 9;
    // block prologue: prove the fast division for the tile, all planes at once
    bool proven = false, dead = false;
    if (FAST) {
        const float x0 = (float)tx0, x1 = (float)min(tx0 + kTileX - 1, tgt_w(g) - 1);
        const float y0 = (float)ty0, y1 = (float)min(ty0 + kTileY - 1, tgt_h(g) - 1);
        bool ok = true, dd = true;
        for (int p = p_begin + (int)threadIdx.x; p < p_end; p += 256) {
            const float* hp = hv + (int64_t)p * 9;
            const bool safe = div2_rect_safe(hp, x0, x1, y0, y1);
            ok = ok && safe;
            dd = dd && safe && tile_dead(hp, x0, x1, y0, y1, g);
        }
        proven = __syncthreads_and(ok);
        dead = __syncthreads_and(dd);
    }
    if (x >= tgt_w(g) || y >= tgt_h(g)) return;
    const int64_t o = ((int64_t)v * tgt_h(g) + y) * tgt_w(g) + x;
    float* out_px = CT ? out + o * 4 : out + o * 3;
    if (dead) {  // every plane samples the zero border over the whole tile
        float cr = -0.0f, cg = -0.0f, cb = -0.0f, t = 1.0f;
        composite_zero<CT>(p_begin, p_end, !CT || back, cr, cg, cb, t);
        if (CT) {
            *reinterpret_cast<float4*>(out_px) = make_float4(cr, cg, cb, t);
        } else {
            out_px[0] = cr;
            out_px[1] = cg;
            out_px[2] = cb;
        }
        return;
    }
    if (!FAST)
        render_packed_pixel<CT, 0>(planes, plane_stride, g, p_begin, p_end, back, hv, x, y, out_px);
    else if (proven)
        render_packed_pixel<CT, 2>(planes, plane_stride, g, p_begin, p_end, back, hv, x, y, out_px);
    else
        render_packed_pixel<CT, 1>(planes, plane_stride, g, p_begin, p_end, back, hv, x, y, out_px);
}

template <bool CT, int R, bool VS = false, bool COUNT = false, int D = 2, bool SAME = false, bool OOB = false>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(SAME && R == 6 && !OOB ? 4 : 1))) void MPIV_KERNEL(render_rows)(const float4* __restrict__ planes, int64_t plane_stride,
                                                          MPIV_GEOM g, int V, int p_begin, int p_end, int back,
                                                          const float* __restrict__ homs, float* __restrict__ out,
                                                          unsigned long long* __restrict__ census = nullptr,
                                                          int y_lo = 0, int y_hi = -1, int colsep = 0,
                                                          int order = 0) {
    constexpr int TY = 4 * R;
    if (y_hi < 0) y_hi = tgt_h(g);
    const int tiles_x = (tgt_w(g) + kTileX - 1) / kTileX;
    const int lb = xcd_logical_block(blockIdx.x, gridDim.x);
    const int v = lb % V;
    // the grid holds the tiles of rows [y_lo, y_hi) once per view (order: xcd_tile_order's)
    const int tile = xcd_tile_order(lb / V, (int)gridDim.x / V, tiles_x, order);
    const int tx0 = (tile % tiles_x) * kTileX, ty0 = y_lo + (tile / tiles_x) * TY;
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
    // column-separable view (ColSet): every plane of the range has h[1] == h[7] == 0.  colsep (the
    // render_colsep option): 0 automatic, -1 never, 1 without the test (a test hook); never where the
    // row pitch does not fit the path's 24-bit tap address (kColsepMaxPitch), the option at 1 included
    // (the (C, T) same-row flavour with R = 8, reached through debug options only, keeps the row
    // recipe: with both row loops it spills two SGPRs)
    constexpr bool COLSEP = VS && !(CT && SAME && R == 8);
    bool sep = false;
    if constexpr (COLSEP)
        sep = g.row < kColsepMaxPitch && (colsep > 0 || (colsep == 0 && __syncthreads_and(cs)));
    if (x >= tgt_w(g) || y0 >= y_hi) return;  // rows past y_hi inside [y0, y0+R) are computed, not stored
    float cr[R], cg[R], cb[R], tt[R];
#pragma unroll
    for (int k = 0; k < R; ++k) {
        cr[k] = -0.0f; cg[k] = -0.0f; cb[k] = -0.0f; tt[k] = 1.0f;  // render_packed_pixel: plane 0 replaces
    }
    if (dead) {  // every plane samples the zero border over the whole tile: no positions, no gathers
        composite_zero<CT>(p_begin, p_end, !CT || back, cr[0], cg[0], cb[0], tt[0]);
#pragma unroll
        for (int k = 1; k < R; ++k) {
            cr[k] = cr[0]; cg[k] = cg[0]; cb[k] = cb[0]; tt[k] = tt[0];
        }
    } else if (!proven) {  // rare (w near 0 over the tile): the guarded one-pixel recipe, row by row
        int rows = 0;
        for (int k = 0; k < R && y0 + k < y_hi; ++k, ++rows) {
            const int64_t o = ((int64_t)v * tgt_h(g) + y0 + k) * tgt_w(g) + x;
            render_packed_pixel<CT, 1>(planes, plane_stride, g, p_begin, p_end, back, hv, x, y0 + k,
                                       CT ? out + o * 4 : out + o * 3);
        }
        // ~(P + 1) issues of 4 gathers per row (render_packed_pixel's ping-pong)
        if (COUNT && (threadIdx.x & (kWave - 1)) == 0)
            atomicAdd(census, (unsigned long long)rows * 4ull * (unsigned long long)(p_end - p_begin + 1));
        return;
    }
    auto store = [&]() {
#pragma unroll
        for (int k = 0; k < R; ++k) {
            const int y = y0 + k;
            if (y >= y_hi) break;
            const int64_t o = ((int64_t)v * tgt_h(g) + y) * tgt_w(g) + x;
            if (CT) {
                reinterpret_cast<float4*>(out)[o] = make_float4(cr[k], cg[k], cb[k], tt[k]);
            } else {
                out[o * 3 + 0] = cr[k];
                out[o * 3 + 1] = cg[k];
                out[o * 3 + 2] = cb[k];
            }
        }
    };
    if (!dead) {
        unsigned nvm = 0;
        if constexpr (VS) {
            if (COLSEP && sep) {  // block-uniform
                render_rows_vs_pixels<CT, false, R, D, SAME, OOB, COLSEP>(planes, plane_stride, g, p_begin, p_end, back, hv,
                                                                        x, y0, cr, cg, cb, tt, nvm);
                if (COUNT && (threadIdx.x & (kWave - 1)) == 0) atomicAdd(census, (unsigned long long)nvm);
                // stored here: with the two row loops' results merged before one store loop, the R
                // rows' colours stay live twice (3R more VGPRs, a wave per SIMD lost)
                store();
                return;
            }
            render_rows_vs_pixels<CT, false, R, D, SAME, OOB>(planes, plane_stride, g, p_begin, p_end, back, hv, x, y0, cr,
                                                              cg, cb, tt, nvm);
        } else  // 4 gathers per issue: R per plane plus the first
            render_rows_pixels<CT, false, R>(planes, plane_stride, g, p_begin, p_end, back, hv, x, y0, cr, cg, cb, tt);
        if (!VS) nvm = 4u * (unsigned)(R * (p_end - p_begin) + 1);
        if (COUNT && (threadIdx.x & (kWave - 1)) == 0) atomicAdd(census, (unsigned long long)nvm);
    }
    store();
}
