// pmx_grid_tile.inc — the wave-cooperative tile search (included by pmx_grid.hip).
//
// One wave = 64 consecutive queries of the slot order (a compact cluster).
// Round 0 takes the bounding box of the wave's query cells grown by one
// cell; every later round grows the box by one more cell.  Each round copies
// only the points the box GAINED (whole rows for rows new to the box, the two
// end cells for rows it already had) from HBM into LDS, coalesced, and every
// lane that is not yet certified scans them with broadcast LDS reads.  A lane
// is certified once its k-th distance is below the squared distance to the
// nearest interior face of the box (LB test, see pmx_grid.hip); the wave
// stops when every lane is certified.  A wave whose box would exceed
// `max_pts` points (or 1024 rows) hands its uncertified lanes to the
// per-lane shell search.
//
// Cold form (kTileCold): the first match of a new reading inside the
// per-lane default mode (nothing to reuse yet, and at the initial pose half
// the queries need shells past the 3x3x3 block, which the per-lane walk pays
// for in dependent gathers).  It takes the device loop's level and transform,
// classifies the quantile window, writes safe radius 0 (the next match does a
// full search or, at the same level, stores fresh radii), counts every query
// as a full search, and reports as visits a per-lane shell-search estimate:
// the points of the lane's 3x3x3 block scaled by the surface area of the cube
// it needed, ((2R + 1) / 3)^2 for R = 1 + growth rounds (the measure the
// level choice reads: the broadcast LDS reads are not per-query work a
// per-lane search at the next level would repeat).

template <typename T>
struct TileCap {
    static constexpr int value = 8192 / (int)sizeof(P4<T>);  // 8 KB of LDS per wave
};

constexpr int kTileMaxRows = 1024;

// float, k = 1: the LDS tile in pair-SoA form so that two points' distances
// take one packed f32 instruction per step (v_pk_add_f32 / v_pk_mul_f32: the
// same IEEE operations per element as gsqd, hence the same bits).  In the 8 KB
// of a CAP-point tile: (x_a, x_b, y_a, y_b) per pair, then (z_a, z_b) per pair,
// then the positions.
template <typename T, int KT>
struct TilePk {
    static constexpr bool value = sizeof(T) == 4 && KT == 1;
};

typedef float pmx_f2 __attribute__((ext_vector_type(2)));

__device__ __forceinline__ void tile_put_pk(float* __restrict__ lds, int cap, int t, float x, float y, float z,
                                            uint32_t pos) {
    const int pr = (t >> 1) * 4 + (t & 1);
    lds[pr] = x;
    lds[pr + 2] = y;
    lds[2 * cap + t] = z;
    reinterpret_cast<uint32_t*>(lds)[3 * cap + t] = pos;
}

__device__ __forceinline__ void tile_scan_pk(const float* __restrict__ lds, int cap, int cnt,
                                             const int32_t* __restrict__ gidx, float qx, float qy, float qz,
                                             float (&kd)[1], int32_t (&ki)[1]) {
    const float4* xy = reinterpret_cast<const float4*>(lds);
    const pmx_f2* zz = reinterpret_cast<const pmx_f2*>(lds + 2 * cap);
    const uint32_t* ps = reinterpret_cast<const uint32_t*>(lds) + 3 * cap;
    const pmx_f2 QX = {qx, qx}, QY = {qy, qy}, QZ = {qz, qz};
    constexpr int SB = 16;  // min-then-rescan sub-block, as tile_scan
    int s = 0;
    for (; s + SB <= cnt; s += SB) {
        float d[SB];
#pragma unroll
        for (int u = 0; u < SB / 2; ++u) {
            const float4 a = xy[(s >> 1) + u];
            const pmx_f2 dx = pmx_f2{a.x, a.y} - QX;
            const pmx_f2 dy = pmx_f2{a.z, a.w} - QY;
            const pmx_f2 dz = zz[(s >> 1) + u] - QZ;
            pmx_f2 r = dx * dx;
            r = r + dy * dy;
            r = r + dz * dz;
            d[2 * u] = r.x;
            d[2 * u + 1] = r.y;
        }
        float m = d[0];
#pragma unroll
        for (int u = 1; u < SB; ++u) m = vmin(m, d[u]);
        if (m <= kd[0]) {
#pragma unroll
            for (int u = 0; u < SB; ++u) consider<float, 1>(gidx, (int32_t)ps[s + u], d[u], kd, ki);
        }
    }
    for (; s < cnt; ++s) {
        const int pr = (s >> 1) * 4 + (s & 1);
        const P4<float> p{lds[pr], lds[pr + 2], lds[2 * cap + s], 0.f};
        consider<float, 1>(gidx, (int32_t)ps[s], gsqd(qx, qy, qz, p), kd, ki);
    }
}

template <typename T, int KT>
__device__ __forceinline__ void tile_scan(const P4<T>* __restrict__ lp, int cnt, const int32_t* __restrict__ gidx,
                                          T qx, T qy, T qz, T (&kd)[KT], int32_t (&ki)[KT]) {
    int s = 0;
    if constexpr (KT == 1) {
        // min-then-rescan: a 16-point sub-block is reduced with min first and
        // rescanned only when it can improve the lane's best (rare once warm)
        constexpr int SB = 16;
        for (; s + SB <= cnt; s += SB) {
            T d[SB];
#pragma unroll
            for (int u = 0; u < SB; ++u) d[u] = gsqd(qx, qy, qz, lp[s + u]);
            T m = d[0];  // IEEE min: a NaN distance never hides a smaller one
#pragma unroll
            for (int u = 1; u < SB; ++u) m = vmin(m, d[u]);
            if (m <= kd[0]) {
#pragma unroll
                for (int u = 0; u < SB; ++u) consider<T, KT>(gidx, (int32_t)w_pos(lp[s + u].w), d[u], kd, ki);
            }
        }
    } else {
        for (; s + 4 <= cnt; s += 4) {
            P4<T> p[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) p[u] = lp[s + u];
#pragma unroll
            for (int u = 0; u < 4; ++u) consider<T, KT>(gidx, (int32_t)w_pos(p[u].w), gsqd(qx, qy, qz, p[u]), kd, ki);
        }
    }
    for (; s < cnt; ++s) {
        const P4<T> p = lp[s];
        consider<T, KT>(gidx, (int32_t)w_pos(p.w), gsqd(qx, qy, qz, p), kd, ki);
    }
}

// (development profile, PMX_TILE_PROF: per cold-form wave its start / end
// real-time stamps, box rounds and points copied; null: off)
__device__ unsigned long long* g_tile_prof = nullptr;

// which form of the tile kernel a launch runs (a run-time value: one
// instantiation serves the three)
enum TileForm : int {
    kTileTable = 0,  // grid_mode 0: the reading's wave table, no reuse state
    kTileCold = 1,   // a reading's first match under reuse (above)
    kTileWarm = 2,   // tile dispatch: a match with a previous one, when LoopCtl::use_tile says so
};

template <typename T, int KT>
__global__ __launch_bounds__(64, (TileWaves<T, KT>::value)) void grid_tile_kernel(const P4<T>* __restrict__ gpts,
                                                       const int32_t* __restrict__ gidx,
                                                       const uint32_t* __restrict__ start, GridGeom G,
                                                       const P4<T>* __restrict__ rd, int64_t N,
                                                       const uint32_t* __restrict__ waves, Mat4<T> Tm, int k,
                                                       T maxR2, uint32_t max_pts, T* __restrict__ out_d,
                                                       int32_t* __restrict__ out_i,
                                                       unsigned long long* __restrict__ visited,
                                                       const T* __restrict__ radii, TileForm form,
                                                       const LoopCtl* __restrict__ ctl,
                                                       const GridDesc<T>* __restrict__ gd, SpecSel* __restrict__ spec,
                                                       T* __restrict__ safe, P4<T>* __restrict__ nbr,
                                                       const P4<T>* __restrict__ nbr_gpn) {
    constexpr int CAP = TileCap<T>::value;
    if (ctl) {  // device loop: transform and level from the device
        if (ctl->done) return;
        if (form == kTileWarm && !ctl->use_tile) return;  // (tile dispatch: the per-lane kernel runs this match)
        const GridDesc<T>& D = gd[ctl->level];
        gpts = D.gpts;
        gidx = D.gidx;
        start = D.start;
        G = D.G;
        if (nbr_gpn) nbr_gpn = D.gpn;
        ctl_transform(ctl, Tm);
    }
    __shared__ P4<T> lp[CAP];
    __shared__ uint32_t s_off[65];
    __shared__ uint32_t s_a1[64], s_l1[64], s_a2[64];
    const int lane = threadIdx.x;
    // this wave's slots: a row of the wave table (<= 64 slots inside one
    // aligned Morton block), or the plain 64-slot chunk without a table
    // (plain block order: the XCD-aware order of the per-lane kernel made the
    // cold form slower, 0.65 -> 0.75 ms at C3)
    const uint32_t wid = blockIdx.x;
    int64_t s_begin = (int64_t)wid * 64, s_end = min(s_begin + 64, N);
    if (waves) {
        s_begin = waves[wid];
        s_end = waves[wid + 1];
    }
    const int64_t j = s_begin + lane;
    const bool active = j < s_end;
    maxR2 = active ? qr2(radii, j, maxR2) : maxR2;  // (this lane's radius)
    T qx = 0, qy = 0, qz = 0;
    double q[3] = {0, 0, 0};
    int c[3] = {0, 0, 0};
    bool ok = false;
    // warm form: would the per-lane kernel's reuse certificate (its cheap
    // bound, pmx_grid.hip grid_lane_kernel) have passed for this query?  The
    // count of the ones that would not is what the step's tile dispatch rule
    // reads, so no per-lane iteration is spent measuring it.
    bool est_pass = false;
    if (active) {
        const P4<T> p = rd[j];
        gxform(Tm, p, qx, qy, qz);
        q[0] = (double)qx;
        q[1] = (double)qy;
        q[2] = (double)qz;
        bool qnan;
        cell_of_q(G, q, c, qnan);
        ok = !qnan;
        if (form == kTileWarm && safe && ctl && ctl->prev_level == ctl->level) {
            const T rs = safe[j], dkp = out_d[j * k + k - 1];
            Mat4<T> Tp;
#pragma unroll
            for (int i = 0; i < 16; ++i) Tp.m[i] = (T)ctl->Tprev[i];
            T ox, oy, oz;
            gxform(Tp, p, ox, oy, oz);
            const double ex = (double)qx - (double)ox, ey = (double)qy - (double)oy, ez = (double)qz - (double)oz;
            const double delta = sqrt(ex * ex + ey * ey + ez * ez) * (1.0 + kReuseMargin);
            const double av = sqrt((double)dkp) * (1.0 + kReuseMargin) + delta;
            const double bv = (double)rs * (1.0 - kReuseMargin) - delta;
            est_pass = rs > (T)0 && dkp < (T)__builtin_huge_val() && av < bv;
        }
    }
    T kd[KT];
    int32_t ki[KT];
#pragma unroll
    for (int s = 0; s < KT; ++s) {
        kd[s] = (T)__builtin_huge_val();
        ki[s] = kNoPos;
    }
    uint32_t visits = 0;
    unsigned long long* prof = form == kTileCold ? g_tile_prof : nullptr;
    const unsigned long long t_start = prof ? __builtin_amdgcn_s_memrealtime() : 0ull;
    uint32_t copied = 0, nround = 0;
    bool done = !ok;  // lanes without a searchable query are done from the start
    double lbc = -1.0;  // distance to the unvisited region when the lane was certified (warm form: safe radius)
    int rounds = 0;   // box growth rounds this lane needed (cold visits estimate)
    bool abort = false;
    // bounding box of the wave's query cells
    int b0[3], b1[3];
    _Pragma("unroll") for (int a = 0; a < 3; ++a) {
        b0[a] = ok ? c[a] : 0x7fffffff;
        b1[a] = ok ? c[a] : -1;
    }
    for (int off = 32; off > 0; off >>= 1)
        _Pragma("unroll") for (int a = 0; a < 3; ++a) {
            b0[a] = min(b0[a], __shfl_xor(b0[a], off));
            b1[a] = max(b1[a], __shfl_xor(b1[a], off));
        }
    if (b1[0] >= 0) {  // wave-uniform: at least one searchable query
        int p0[3] = {0, 0, 0}, p1[3] = {-1, -1, -1};  // previous box (empty)
        _Pragma("unroll") for (int a = 0; a < 3; ++a) {
            b0[a] = max(b0[a] - 1, 0);
            b1[a] = min(b1[a] + 1, G.g[a] - 1);
        }
        uint32_t budget = max_pts;
        for (;;) {
            const int ny = b1[1] - b0[1] + 1, nz = b1[2] - b0[2] + 1;
            const int nrows = ny * nz;
            if (nrows > kTileMaxRows) {
                abort = true;
                break;
            }
            for (int rb = 0; rb < nrows; rb += 64) {
                // this lane's row: the whole row if it is new to the box,
                // else the cells the box gained at both ends
                uint32_t a1 = 0, l1 = 0, a2 = 0, l2 = 0;
                const int r = rb + lane;
                if (r < nrows) {
                    const int y = b0[1] + r % ny, z = b0[2] + r / ny;
                    const int64_t row = ((int64_t)z * G.g[1] + y) * G.g[0];
                    const bool had = y >= p0[1] && y <= p1[1] && z >= p0[2] && z <= p1[2];
                    if (!had) {
                        a1 = start[row + b0[0]];
                        l1 = start[row + b1[0] + 1] - a1;
                    } else {
                        if (b0[0] < p0[0]) {
                            a1 = start[row + b0[0]];
                            l1 = start[row + p0[0]] - a1;
                        }
                        if (b1[0] > p1[0]) {
                            a2 = start[row + p1[0] + 1];
                            l2 = start[row + b1[0] + 1] - a2;
                        }
                    }
                }
                uint32_t incl = l1 + l2;
                for (int off = 1; off < 64; off <<= 1) {
                    const uint32_t v = __shfl_up(incl, off);
                    if (lane >= off) incl += v;
                }
                const uint32_t total = __shfl(incl, 63);
                if (total > budget) {
                    abort = true;
                    break;
                }
                budget -= total;
                copied += total;
                if (total == 0) continue;
                s_off[lane + 1] = incl;
                if (lane == 0) s_off[0] = 0;
                s_a1[lane] = a1;
                s_l1[lane] = l1;
                s_a2[lane] = a2;
                __syncthreads();
                const int nseg = min(64, nrows - rb);
                for (uint32_t base = 0; base < total; base += CAP) {
                    const int cnt = (int)min((uint32_t)CAP, total - base);
                    // copy: U independent loads in flight per lane
                    constexpr int U = 8;
                    for (int t0 = 0; t0 < cnt; t0 += 64 * U) {
                        // positions first, then all loads, then all LDS stores
                        // (scalar arrays so they stay in registers)
                        uint32_t pos[U];
#pragma unroll
                        for (int u = 0; u < U; ++u) {
                            const uint32_t idx = base + (uint32_t)(t0 + u * 64 + lane);
                            int sg = 0;  // last segment whose offset is <= idx
#pragma unroll
                            for (int st = 32; st > 0; st >>= 1)
                                if (sg + st < nseg && s_off[sg + st] <= idx) sg += st;
                            const uint32_t loc = idx - s_off[sg];
                            const uint32_t l1s = s_l1[sg];
                            pos[u] = loc < l1s ? s_a1[sg] + loc : s_a2[sg] + (loc - l1s);
                        }
                        T vx[U], vy[U], vz[U];
#pragma unroll
                        for (int u = 0; u < U; ++u) {
                            const bool in = t0 + u * 64 + lane < cnt;
                            const P4<T> p = gpts[in ? pos[u] : s_a1[0]];  // in-range dummy address
                            vx[u] = p.x;
                            vy[u] = p.y;
                            vz[u] = p.z;
                        }
#pragma unroll
                        for (int u = 0; u < U; ++u) {
                            const int t = t0 + u * 64 + lane;
                            if constexpr (TilePk<T, KT>::value) {
                                if (t < cnt) tile_put_pk(reinterpret_cast<float*>(lp), CAP, t, vx[u], vy[u], vz[u], pos[u]);
                            } else {
                                if (t < cnt) lp[t] = P4<T>{vx[u], vy[u], vz[u], pos_w(pos[u], T(0))};
                            }
                        }
                    }
                    __syncthreads();
                    if constexpr (TilePk<T, KT>::value) {
                        if (!done) tile_scan_pk(reinterpret_cast<const float*>(lp), CAP, cnt, gidx, qx, qy, qz, kd, ki);
                    } else {
                        if (!done) tile_scan<T, KT>(lp, cnt, gidx, qx, qy, qz, kd, ki);
                    }
                    __syncthreads();
                }
                if (!done) visits += total;
            }
            if (abort) break;
            // certification against the interior faces of the box
            if (!done) {
                const double margin = 1.0 - 1e-5;
                double lb = 1e300;
                bool any = false;
                _Pragma("unroll") for (int a = 0; a < 3; ++a) {
                    if (b0[a] > 0) {
                        lb = fmin(lb, q[a] - (G.lo[a] + (double)b0[a] * G.h));
                        any = true;
                    }
                    if (b1[a] < G.g[a] - 1) {
                        lb = fmin(lb, (G.lo[a] + (double)(b1[a] + 1) * G.h) - q[a]);
                        any = true;
                    }
                }
                if (!any) {
                    done = true;  // the box is the whole grid
                    lbc = 1e300;
                } else if (lb > 0.0) {
                    const double lb2 = lb * lb * margin;
                    T dk;
                    int32_t ik;
                    kth(kd, ki, k, dk, ik);  // (KT >= k: certified on the k-th entry)
                    if (((double)dk < lb2 && ik != kNoPos) || lb2 > (double)maxR2) {
                        done = true;
                        lbc = lb;
                    }
                }
            }
            ++nround;
            if (__ballot(!done) == 0) break;
            if (!done) ++rounds;
            // grow the box by one cell (it is not the whole grid: some lane
            // still saw an interior face)
            _Pragma("unroll") for (int a = 0; a < 3; ++a) {
                p0[a] = b0[a];
                p1[a] = b1[a];
                b0[a] = max(b0[a] - 1, 0);
                b1[a] = min(b1[a] + 1, G.g[a] - 1);
            }
        }
    }
    const bool fallback = abort && !done;
    if (prof) {
        const unsigned long long nfb_lanes = __popcll(__ballot(fallback));
        if (lane == 0) {
            const unsigned long long t_end = __builtin_amdgcn_s_memrealtime();
            prof[4 * wid] = t_start;
            prof[4 * wid + 1] = t_end;
            prof[4 * wid + 2] = nround | (nfb_lanes << 32);
            prof[4 * wid + 3] = copied;
        }
    }
    {
        const unsigned long long nfb = __popcll(__ballot(fallback));
        if (lane == 0 && nfb && visited && form == kTileTable) atomicAdd(vslot(visited, 1), nfb);
    }
    if (fallback) {
        if (form != kTileTable) visits = 0;  // (a cold or warm fallback lane reports its own walk)
#pragma unroll
        for (int s = 0; s < KT; ++s) {
            kd[s] = (T)__builtin_huge_val();
            ki[s] = kNoPos;
        }
        double lbx;
        lane_search<T, KT>(gpts, gidx, start, G, qx, qy, qz, q, c, maxR2, k, kd, ki, visits, lbx);
        lbc = lbx;
    }
    if (form == kTileTable) {
        if (active) write_out<T, KT>(j, k, maxR2, kd, ki, out_d, out_i);
        add_visits(visits, visited);
        return;
    }
    SpecAcc<T> sa;
    spec_acc_init<T>(sa, spec);
    if (active) {
        write_out<T, KT>(j, k, maxR2, kd, ki, out_d, out_i, sa);
        // (the cold form keeps k entries: radius 0, the next match searches;
        // the warm form's lists hold the (k+1)-th: the safe radius of the
        // box it was certified in, as a per-lane search leaves it)
        if (safe) st_out(&safe[j], form == kTileWarm ? safe_radius<T, KT>(kd, ki, k, lbc) : (T)0);
        if (safe && k == 1) write_nbr<T, KT>(nbr, gpts, nbr_gpn, N, j, maxR2, kd, ki);
    }
    // lane-search-equivalent visits: the points of the lane's 3x3x3 block
    // (plus a fallback lane's own walk, already in `visits`)
    uint32_t blk = 0;
    if (ok) {
        const int x0 = max(c[0] - 1, 0), x1 = min(c[0] + 1, G.g[0] - 1);
#pragma unroll
        for (int r = 0; r < 9; ++r) {
            const int z = c[2] + r / 3 - 1, y = c[1] + r % 3 - 1;
            if (z >= 0 && z < G.g[2] && y >= 0 && y < G.g[1]) {
                const uint32_t row = ((uint32_t)z * (uint32_t)G.g[1] + (uint32_t)y) * (uint32_t)G.g[0];
                blk += gld32(start, row + x1 + 1) - gld32(start, row + x0);
            }
        }
    }
    const float grow = (float)(2 * rounds + 3) * (1.0f / 3.0f);
    add_visits(fallback ? visits : (uint32_t)((float)blk * grow * grow), visited);
    if (prof && lane == 0)  // (high word: the wave's end after its fallback walks, ticks after t_start)
        prof[4 * wid + 3] = copied | ((__builtin_amdgcn_s_memrealtime() - t_start) << 32);
    {
        // (full searches: every query; the warm form counts the ones the
        // per-lane certificate would have failed)
        const unsigned long long m = __ballot(active && !(form == kTileWarm && est_pass));
        if (lane == 0 && visited && safe && m) atomicAdd(vslot(visited, 1), (unsigned long long)__popcll(m));
    }
    if (sa.on) spec_acc_flush<T>(sa, vslot(visited, 2), vslot(visited, 3));
}
