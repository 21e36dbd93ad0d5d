// Exact geodesic disks for the evaluator (gfx950): the membership test of the reference's CGAL tool, evaluation_code/evaluation.cpp
// :85-115 (Surface_mesh_shortest_path with one source per seed, shortest_distance_to_source_points for every projected point that
// passes the straight-line pre-filter at :95).
//
// One workgroup per seed runs Chen & Han's window propagation (continuous Dijkstra on the unfolded surface) in parallel rounds, as in
// Ying, Xin & He, "Parallel Chen-Han (PCH) algorithm for discrete geodesics" (ACM TOG 33(1), 2014), bounded by max_dist:
//   * a window is an interval [b0, b1] of an edge lit by straight lines from one unfolded source image I = (ix, iy < 0) at geodesic
//     distance sigma, stored in the frame of the face it lights (edge k of face f: f[k] at the origin, f[k+1] at (L, 0), the third
//     vertex at (cx, cy > 0); dis-pu_amd/mesh.py:geodesic_tables).  A window whose lower bound sigma + dist(I, interval) exceeds
//     max_dist is dropped;
//   * round r propagates every window of round r-1 across its face into at most two children (split at the opposite vertex, which
//     the window then reaches) and relaxes the vertices it reaches (LDS atomic min on the fp64 bits: min is order-free);
//   * Xin & Wang's filter ("Improving Chen and Han's algorithm on the discrete geodesic problem", ACM TOG 28(4), 2009) drops a new
//     window on edge (P, Q) when d(P) + |P B1| < sigma + |I B1| at its far end (or the same from Q at the near end): |I x| - |P x| does
//     not grow along the edge, so the path over P then beats the window at every point of it.  The vertex distances it reads are a
//     snapshot taken between rounds, so the surviving window SET does not depend on scheduling (only its order in the arena does,
//     and every output is a minimum over that set: bit-identical run to run);
//   * between rounds, a saddle (angle sum >= 2 pi) or boundary vertex whose distance improved is a pseudo-source: it emits windows
//     onto the edges opposite it in its fan;
//   * a target t in face f then takes the least of |s - t| (f holds the seed), d(v) + |v - t| over f's vertices, and over f's windows
//     sigma + |I - t| if t is seen through [b0, b1], else sigma + the path over the nearer window end.  Each is a real path length,
//     so nothing undercuts the geodesic.
// All geometry is fp64.  Vertex distances live in an LDS hash (vertex id -> slot); windows in a per-seed arena in the caller's
// scratch.  An arena or hash that overflows sets the seed's status and its distances are not written: the caller reruns the seed
// with a larger arena (dis-pu_amd/mesh.py), nothing is truncated.
#include "common.h"
#include "internal.h"

namespace dispu {
constexpr int GEO_BS = 256;
constexpr int GEO_TCH = 1024;            // targets per evaluation pass (LDS)
constexpr int GEO_HMIN = 512, GEO_HMAX = 4096;
constexpr double GEO_TOL = 1e-12;
constexpr unsigned long long GEO_INF = 0x7FF0000000000000ull;

struct Win {
    double sigma, ix, iy, b0, b1;
    int he;          // f*3 + k: lights face f through its edge k
    int pad;
};

__host__ __device__ inline int geo_hash_slots(int window_cap) {
    int h = GEO_HMIN;
    while (h < GEO_HMAX && h < window_cap / 4) h <<= 1;
    return h;
}

struct GeoCtx {
    const double* V;
    const int* Fc;
    const int* twin;
    const double* geo;
    const int* pseudo;
    int* keys;                    // LDS, -1 = empty
    unsigned long long* ucur;     // LDS, fp64 bits of the best path length found so far
    unsigned long long* uold;     // LDS, the snapshot the filter and the pseudo-sources read
    unsigned long long* uemit;    // LDS, the distance a pseudo-source last emitted with
    int H;
    Win* win;
    int W;
    int* count;                   // LDS
    int* flags;                   // LDS: 1 arena full, 2 hash full
    double maxd;
};

__device__ __forceinline__ double geo_len(double x, double y) { return sqrt(x * x + y * y); }
__device__ __forceinline__ double geo_cross(double ax, double ay, double bx, double by) { return ax * by - ay * bx; }
__device__ __forceinline__ unsigned long long dbits(double d) { return (unsigned long long)__double_as_longlong(d); }
__device__ __forceinline__ double bitsd(unsigned long long b) { return __longlong_as_double((long long)b); }

__device__ __forceinline__ unsigned geo_h(int key, int H) { return ((unsigned)key * 2654435761u) & (unsigned)(H - 1); }

__device__ int geo_find(const GeoCtx& c, int key) {
    unsigned s = geo_h(key, c.H);
    for (int p = 0; p < c.H; ++p, s = (s + 1) & (unsigned)(c.H - 1)) {
        const int k = __hip_atomic_load(&c.keys[s], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        if (k == key) return (int)s;
        if (k < 0) return -1;
    }
    return -1;
}

__device__ int geo_insert(const GeoCtx& c, int key) {
    unsigned s = geo_h(key, c.H);
    for (int p = 0; p < c.H; ++p, s = (s + 1) & (unsigned)(c.H - 1)) {
        int k = __hip_atomic_load(&c.keys[s], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        if (k < 0) k = atomicCAS(&c.keys[s], -1, key);
        if (k < 0 || k == key) return (int)s;
    }
    atomicOr(c.flags, 2);
    return -1;
}

__device__ __forceinline__ double geo_uold(const GeoCtx& c, int v) {
    const int s = geo_find(c, v);
    return s < 0 ? bitsd(GEO_INF) : bitsd(c.uold[s]);
}

__device__ void geo_relax(const GeoCtx& c, int v, double d) {
    if (!(d <= c.maxd)) return;
    const int s = geo_insert(c, v);
    if (s >= 0) atomicMin(&c.ucur[s], dbits(d));
}

// A window on edge k of face f lighting the face across it: source (x, y > 0) and [lo, hi] in f's frame of edge k.  Stored in the
// twin's frame, where the lit face is at +y and the source below.
__device__ void geo_push(const GeoCtx& c, int f, int k, double sigma, double x, double y, double lo, double hi) {
    const int t = c.twin[f * 3 + k];
    if (t < 0) return;
    const int g = t / 3, kk = t - 3 * g;
    const double L = c.geo[(f * 3 + k) * 3];
    const bool same = c.Fc[g * 3 + kk] == c.Fc[f * 3 + k];      // a badly oriented neighbour: the edge runs the same way
    const double jx = same ? x : L - x, jy = -y;
    double c0 = same ? lo : L - hi, c1 = same ? hi : L - lo;
    c0 = fmax(c0, 0.0);
    c1 = fmin(c1, L);
    if (!(c1 - c0 > GEO_TOL * L) || !(jy < -GEO_TOL * L)) return;
    const double lb = sigma + geo_len(fmin(fmax(jx, c0), c1) - jx, jy);
    if (lb > c.maxd) return;
    // Xin-Wang filter against the snapshot of the edge's endpoint distances
    const int P = c.Fc[g * 3 + kk], Q = c.Fc[g * 3 + (kk == 2 ? 0 : kk + 1)];
    const double far = sigma + geo_len(c1 - jx, jy), near = sigma + geo_len(c0 - jx, jy);
    if (geo_uold(c, P) + c1 < far * (1.0 - GEO_TOL)) return;
    if (geo_uold(c, Q) + (L - c0) < near * (1.0 - GEO_TOL)) return;
    const int at = atomicAdd(c.count, 1);
    if (at >= c.W) { atomicOr(c.flags, 1); return; }
    Win w;
    w.sigma = sigma; w.ix = jx; w.iy = jy; w.b0 = c0; w.b1 = c1; w.he = t; w.pad = 0;
    c.win[at] = w;
}

// rays from I through (x0, 0), (x1, 0) onto edge kk = P -> Q of face f (2D points of the current frame; R the third vertex)
__device__ void geo_child(const GeoCtx& c, int f, int kk, double px, double py, double qx, double qy, double rx, double ry, double sigma,
                          double ix, double iy, double x0, double x1) {
    const double ex = qx - px, ey = qy - py;
    const double Lpq = geo_len(ex, ey);
    const double ux = ex / Lpq, uy = ey / Lpq;
    const double sg = geo_cross(ux, uy, rx - px, ry - py) > 0.0 ? 1.0 : -1.0;
    double h[2];
    const double xs[2] = {x0, x1};
    for (int e = 0; e < 2; ++e) {
        const double dx = xs[e] - ix, dy = -iy;
        const double den = geo_cross(ex, ey, dx, dy);
        if (fabs(den) <= 1e-300) return;                             // a ray along the edge: nothing crosses it
        const double s = geo_cross(ix - px, iy - py, dx, dy) / den;
        h[e] = fmin(fmax(s, 0.0), 1.0) * Lpq;
    }
    const double jx = (ix - px) * ux + (iy - py) * uy;
    const double jy = sg * geo_cross(ux, uy, ix - px, iy - py);
    geo_push(c, f, kk, sigma, jx, jy, fmin(h[0], h[1]), fmax(h[0], h[1]));
}

__device__ void geo_propagate(const GeoCtx& c, const Win& w) {
    const int f = w.he / 3, k = w.he - 3 * (w.he / 3);
    const int k1 = k == 2 ? 0 : k + 1, k2 = k == 0 ? 2 : k - 1;
    const double* gk = c.geo + (f * 3 + k) * 3;
    const double L = gk[0], cx = gk[1], cy = gk[2];
    const double ix = w.ix, iy = w.iy, b0 = w.b0, b1 = w.b1, sigma = w.sigma;
    const double xc = ix + (cx - ix) * (-iy) / (cy - iy);
    if (b0 < xc && xc < b1) geo_relax(c, c.Fc[f * 3 + k2], sigma + geo_len(cx - ix, cy - iy));
    if (b0 <= GEO_TOL * L) geo_relax(c, c.Fc[f * 3 + k], sigma + geo_len(ix, iy));
    if (b1 >= L * (1.0 - GEO_TOL)) geo_relax(c, c.Fc[f * 3 + k1], sigma + geo_len(L - ix, iy));
    if (b0 < xc) geo_child(c, f, k2, cx, cy, 0.0, 0.0, L, 0.0, sigma, ix, iy, b0, fmin(b1, xc));   // onto edge c -> a
    if (xc < b1) geo_child(c, f, k1, L, 0.0, cx, cy, 0.0, 0.0, sigma, ix, iy, fmax(b0, xc), b1);   // onto edge b -> c
}

__device__ __forceinline__ double geo_dist3(const double* V, int v, double x, double y, double z) {
    const double dx = V[3 * v] - x, dy = V[3 * v + 1] - y, dz = V[3 * v + 2] - z;
    return sqrt((dx * dx + dy * dy) + dz * dz);
}

// a pseudo-source v at distance u: windows onto the edges opposite v in its fan, and its fan neighbours relaxed
__device__ void geo_emit_vertex(const GeoCtx& c, const long long* fan_off, const int* fan, int v, double u) {
    const double vx = c.V[3 * v], vy = c.V[3 * v + 1], vz = c.V[3 * v + 2];
    for (long long e = fan_off[v]; e < fan_off[v + 1]; ++e) {
        const int f = fan[e] / 3, j = fan[e] - 3 * (fan[e] / 3);
        const int k = j == 2 ? 0 : j + 1;
        const double* gk = c.geo + (f * 3 + k) * 3;
        geo_push(c, f, k, u, gk[1], gk[2], 0.0, gk[0]);
        const int a = c.Fc[f * 3 + k], b = c.Fc[f * 3 + (k == 2 ? 0 : k + 1)];
        geo_relax(c, a, u + geo_dist3(c.V, a, vx, vy, vz));
        geo_relax(c, b, u + geo_dist3(c.V, b, vx, vy, vz));
    }
}

// (x, y) of p in face f's frame of edge k
__device__ __forceinline__ void geo_to2d(const GeoCtx& c, int f, int k, double px, double py, double pz, double& x, double& y) {
    const int a = c.Fc[f * 3 + k], b = c.Fc[f * 3 + (k == 2 ? 0 : k + 1)], d = c.Fc[f * 3 + (k == 0 ? 2 : k - 1)];
    const double* gk = c.geo + (f * 3 + k) * 3;
    const double L = gk[0], cx = gk[1], cy = gk[2];
    const double ax = c.V[3 * a], ay = c.V[3 * a + 1], az = c.V[3 * a + 2];
    const double exx = (c.V[3 * b] - ax) / L, exy = (c.V[3 * b + 1] - ay) / L, exz = (c.V[3 * b + 2] - az) / L;
    const double eyx = (c.V[3 * d] - ax - cx * exx) / cy, eyy = (c.V[3 * d + 1] - ay - cx * exy) / cy, eyz = (c.V[3 * d + 2] - az - cx * exz) / cy;
    const double qx = px - ax, qy = py - ay, qz = pz - az;
    x = (qx * exx + qy * exy) + qz * exz;
    y = (qx * eyx + qy * eyy) + qz * eyz;
}

__global__ __launch_bounds__(GEO_BS) void geodesic_kernel(const int* __restrict__ seed_face, const double* __restrict__ seed_bary,
                                                          const double* __restrict__ V, const int* __restrict__ Fc,
                                                          const int* __restrict__ twin, const double* __restrict__ geo,
                                                          const int* __restrict__ pseudo, const long long* __restrict__ fan_off,
                                                          const int* __restrict__ fan, const float* __restrict__ points,
                                                          const int* __restrict__ point_face, const long long* __restrict__ cand_off,
                                                          const int* __restrict__ cand, double maxd, int W, int H, Win* __restrict__ arena,
                                                          double* __restrict__ dist, int* __restrict__ status) {
    extern __shared__ __align__(16) unsigned char geo_lds[];
    unsigned long long* ucur = reinterpret_cast<unsigned long long*>(geo_lds);
    unsigned long long* uold = ucur + H;
    unsigned long long* uemit = uold + H;
    unsigned long long* best = uemit + H;                         // [GEO_TCH]
    int* keys = reinterpret_cast<int*>(best + GEO_TCH);
    int* tface = keys + H;                                        // [GEO_TCH]: sorted target faces
    int* tidx = tface + GEO_TCH;                                  // [GEO_TCH]: their local target index
    int* tf_raw = tidx + GEO_TCH;                                 // [GEO_TCH]
    __shared__ int count, flags, n_src, src_face[2], round_hi, round_flags;
    __shared__ double sp[3];
    const int i = blockIdx.x, tid = threadIdx.x;
    for (int s = tid; s < H; s += GEO_BS) { keys[s] = -1; ucur[s] = GEO_INF; uold[s] = GEO_INF; uemit[s] = GEO_INF; }
    if (tid == 0) { count = 0; flags = 0; }
    __syncthreads();
    GeoCtx c;
    c.V = V; c.Fc = Fc; c.twin = twin; c.geo = geo; c.pseudo = pseudo;
    c.keys = keys; c.ucur = ucur; c.uold = uold; c.uemit = uemit; c.H = H;
    c.win = arena + (size_t)i * W; c.W = W; c.count = &count; c.flags = &flags; c.maxd = maxd;
    if (tid == 0) {
        const int fs = seed_face[i];
        const double b[3] = {seed_bary[3 * i], seed_bary[3 * i + 1], seed_bary[3 * i + 2]};
        double s[3];
        for (int d = 0; d < 3; ++d)
            s[d] = (b[0] * V[3 * Fc[3 * fs] + d] + b[1] * V[3 * Fc[3 * fs + 1] + d]) + b[2] * V[3 * Fc[3 * fs + 2] + d];
        sp[0] = s[0]; sp[1] = s[1]; sp[2] = s[2];
        const int nz = (b[0] == 0.0) + (b[1] == 0.0) + (b[2] == 0.0);
        src_face[0] = src_face[1] = -1;
        n_src = 0;
        if (nz >= 2) {                                           // on a vertex: a pseudo-source at distance 0
            const int v = Fc[3 * fs + (b[0] != 0.0 ? 0 : (b[1] != 0.0 ? 1 : 2))];
            const int sl = geo_insert(c, v);
            if (sl >= 0) { ucur[sl] = 0; uemit[sl] = 0; }
            geo_emit_vertex(c, fan_off, fan, v, 0.0);
        } else {
            src_face[n_src++] = fs;
            if (nz == 1) {                                       // on an edge: the face across holds the seed too
                const int j = b[0] == 0.0 ? 0 : (b[1] == 0.0 ? 1 : 2);
                const int t = twin[3 * fs + (j == 2 ? 0 : j + 1)];
                if (t >= 0) src_face[n_src++] = t / 3;
            }
            for (int q = 0; q < n_src; ++q) {
                const int f = src_face[q];
                for (int k = 0; k < 3; ++k) {
                    const int v = Fc[3 * f + k];
                    geo_relax(c, v, geo_dist3(V, v, s[0], s[1], s[2]));
                    double x, y;
                    geo_to2d(c, f, k, s[0], s[1], s[2], x, y);
                    const double L = geo[(f * 3 + k) * 3];
                    if (y > GEO_TOL * L) geo_push(c, f, k, 0.0, x, y, 0.0, L);
                }
            }
        }
    }
    __syncthreads();
    int lo = 0;
    for (;;) {
        // between rounds: snapshot the vertex distances, then let the pseudo-sources that improved emit
        for (int s = tid; s < H; s += GEO_BS) uold[s] = ucur[s];
        __syncthreads();
        for (int s = tid; s < H; s += GEO_BS) {
            const int v = __hip_atomic_load(&keys[s], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
            if (v >= 0 && pseudo[v] && uold[s] < uemit[s] && bitsd(uold[s]) <= maxd) {
                uemit[s] = uold[s];
                geo_emit_vertex(c, fan_off, fan, v, bitsd(uold[s]));
            }
        }
        __syncthreads();
        if (tid == 0) { round_hi = min(count, W); round_flags = flags; }
        __syncthreads();
        const int hi = round_hi;                                 // read by every thread before any appends again
        if (round_flags || lo >= hi) break;
        for (int w = lo + tid; w < hi; w += GEO_BS) geo_propagate(c, c.win[w]);
        lo = hi;
        __syncthreads();
    }
    if (round_flags) {
        if (tid == 0) status[i] = round_flags;
        return;
    }
    const int nw = lo;
    const long long cb = cand_off[i], ce = cand_off[i + 1];
    for (long long c0 = cb; c0 < ce; c0 += GEO_TCH) {
        const int nt = (int)min((long long)GEO_TCH, ce - c0);
        for (int t = tid; t < nt; t += GEO_BS) tf_raw[t] = point_face[cand[c0 + t]];
        __syncthreads();
        for (int t = tid; t < nt; t += GEO_BS) {                 // rank sort by (face, index)
            const int ft = tf_raw[t];
            int r = 0;
            for (int u = 0; u < nt; ++u) r += (tf_raw[u] < ft) || (tf_raw[u] == ft && u < t);
            tface[r] = ft;
            tidx[r] = t;
            // the seed's own face(s) and the vertices of the target's face
            const int q = cand[c0 + t];
            const double px = points[3 * q], py = points[3 * q + 1], pz = points[3 * q + 2];
            double d = bitsd(GEO_INF);
            if (ft == src_face[0] || ft == src_face[1]) {
                const double dx = px - sp[0], dy = py - sp[1], dz = pz - sp[2];
                d = sqrt((dx * dx + dy * dy) + dz * dz);
            }
            for (int k = 0; k < 3; ++k) {
                const int v = Fc[3 * ft + k];
                const int sl = geo_find(c, v);
                if (sl >= 0 && ucur[sl] != GEO_INF) d = fmin(d, bitsd(ucur[sl]) + geo_dist3(V, v, px, py, pz));
            }
            best[t] = dbits(d);
        }
        __syncthreads();
        for (int w = tid; w < nw; w += GEO_BS) {
            const Win win = c.win[w];
            const int f = win.he / 3, k = win.he - 3 * (win.he / 3);
            int a = 0, b = nt;                                   // first sorted target of face f
            while (a < b) {
                const int m = (a + b) >> 1;
                if (tface[m] < f) a = m + 1; else b = m;
            }
            for (int r = a; r < nt && tface[r] == f; ++r) {
                const int t = tidx[r];
                const int q = cand[c0 + t];
                double tx, ty;
                geo_to2d(c, f, k, points[3 * q], points[3 * q + 1], points[3 * q + 2], tx, ty);
                const double x = ty - win.iy > 0.0 ? win.ix + (tx - win.ix) * (-win.iy) / (ty - win.iy) : __builtin_nan("");
                double d;
                if (win.b0 <= x && x <= win.b1)
                    d = win.sigma + geo_len(tx - win.ix, ty - win.iy);
                else
                    d = win.sigma + fmin(geo_len(win.b0 - win.ix, win.iy) + geo_len(tx - win.b0, ty),
                                         geo_len(win.b1 - win.ix, win.iy) + geo_len(tx - win.b1, ty));
                atomicMin(&best[t], dbits(d));
            }
        }
        __syncthreads();
        for (int t = tid; t < nt; t += GEO_BS) {
            const double d = bitsd(best[t]);
            dist[c0 + t] = d <= maxd ? d : bitsd(GEO_INF);
        }
        __syncthreads();
    }
    if (tid == 0) status[i] = 0;
}

__device__ __forceinline__ bool geo_in(const double* dist, long long c, double r) { return dist[c] <= r; }

// offsets[1 + i*R + j] = |{candidates c of seed i : dist[c] <= (double)radii[j]}|; one wave per seed
constexpr int GEO_SEL_WAVES = 4;
__global__ __launch_bounds__(64 * GEO_SEL_WAVES) void geo_count_kernel(int S, int R, const long long* __restrict__ cand_off,
                                                                       const double* __restrict__ dist, const float* __restrict__ radii,
                                                                       long long* __restrict__ offsets) {
    const int lane = threadIdx.x & 63;
    const int i = blockIdx.x * GEO_SEL_WAVES + (threadIdx.x >> 6);
    if (i >= S) return;
    const long long b = cand_off[i], e = cand_off[i + 1];
    for (int j = 0; j < R; ++j) {
        const double r = (double)radii[j];
        long long cnt = 0;
        for (long long c0 = b; c0 < e; c0 += 64) {
            const long long c = c0 + lane;
            cnt += __popcll(__ballot(c < e && geo_in(dist, c, r)));
        }
        if (lane == 0) offsets[1 + (long long)i * R + j] = cnt;
    }
}

__global__ __launch_bounds__(64 * GEO_SEL_WAVES) void geo_fill_kernel(int S, int R, const long long* __restrict__ cand_off,
                                                                      const int* __restrict__ cand, const double* __restrict__ dist,
                                                                      const float* __restrict__ radii, const long long* __restrict__ offsets,
                                                                      int* __restrict__ members) {
    const int lane = threadIdx.x & 63;
    const int i = blockIdx.x * GEO_SEL_WAVES + (threadIdx.x >> 6);
    if (i >= S) return;
    const long long b = cand_off[i], e = cand_off[i + 1];
    for (int j = 0; j < R; ++j) {
        const double r = (double)radii[j];
        const long long k = (long long)i * R + j, end = offsets[k + 1];
        long long pos = offsets[k];
        for (long long c0 = b; c0 < e && pos < end; c0 += 64) {
            const long long c = c0 + lane;
            const bool in = c < e && geo_in(dist, c, r);
            const uint64_t m = __ballot(in);
            const long long at = pos + __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
            if (in && at < end) members[at] = cand[c];
            pos += __popcll(m);
        }
    }
}

}  // namespace dispu

using namespace dispu;

static size_t geo_lds_bytes(int H) {
    return (size_t)H * (3 * sizeof(unsigned long long) + sizeof(int)) + (size_t)GEO_TCH * (sizeof(unsigned long long) + 3 * sizeof(int));
}

DISPU_EXPORT size_t dispu_geodesic_scratch_bytes(int S, int window_cap) {
    if (S <= 0 || window_cap <= 0) return 0;
    return (size_t)S * (size_t)window_cap * sizeof(Win);
}

DISPU_EXPORT int dispu_geodesic_hash_slots(int window_cap) { return window_cap > 0 ? geo_hash_slots(window_cap) : 0; }

DISPU_EXPORT int dispu_geodesic_distances(int S, const int* seed_face, const double* seed_bary, const double* verts, const int* faces,
                                          const int* twin, const double* edge_geo, const int* pseudo, const long long* fan_off,
                                          const int* fan, int n, const float* points, const int* point_face, const long long* cand_off,
                                          const int* cand, double max_dist, int window_cap, void* scratch, size_t scratch_bytes,
                                          double* dist, int* status, void* stream) {
    if (S < 0 || n <= 0 || window_cap <= 0 || !(max_dist >= 0.0)) return (int)hipErrorInvalidValue;
    if (S == 0) return 0;
    if (!scratch || scratch_bytes < dispu_geodesic_scratch_bytes(S, window_cap)) return (int)hipErrorInvalidValue;
    const int H = geo_hash_slots(window_cap);
    static bool attr = false;
    if (!attr) {
        DISPU_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(geodesic_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                      (int)geo_lds_bytes(GEO_HMAX)));
        attr = true;
    }
    hipLaunchKernelGGL(geodesic_kernel, dim3(S), dim3(GEO_BS), geo_lds_bytes(H), (hipStream_t)stream, seed_face, seed_bary, verts, faces,
                       twin, edge_geo, pseudo, fan_off, fan, points, point_face, cand_off, cand, max_dist, window_cap, H,
                       static_cast<Win*>(scratch), dist, status);
    return (int)hipGetLastError();
}

DISPU_EXPORT int dispu_geodesic_disk_count(int S, int R, const long long* cand_off, const double* dist, const float* radii,
                                           long long* offsets, void* stream) {
    if (S < 0 || R <= 0) return (int)hipErrorInvalidValue;
    hipStream_t st = (hipStream_t)stream;
    if (S == 0) return (int)hipMemsetAsync(offsets, 0, sizeof(long long), st);
    hipLaunchKernelGGL(geo_count_kernel, dim3((S + GEO_SEL_WAVES - 1) / GEO_SEL_WAVES), dim3(64 * GEO_SEL_WAVES), 0, st, S, R, cand_off,
                       dist, radii, offsets);
    DISPU_CHECK_LAUNCH();
    return disk_scan_launch((long long)S * R, offsets, st);
}

DISPU_EXPORT int dispu_geodesic_disk_fill(int S, int R, const long long* cand_off, const int* cand, const double* dist, const float* radii,
                                          const long long* offsets, int* members, void* stream) {
    if (S < 0 || R <= 0) return (int)hipErrorInvalidValue;
    if (S == 0) return 0;
    hipLaunchKernelGGL(geo_fill_kernel, dim3((S + GEO_SEL_WAVES - 1) / GEO_SEL_WAVES), dim3(64 * GEO_SEL_WAVES), 0, (hipStream_t)stream, S,
                       R, cand_off, cand, dist, radii, offsets, members);
    return (int)hipGetLastError();
}
