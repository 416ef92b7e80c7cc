// racinglmpc_amd/csrc/lmpc_track.hip.h -- the inverse half of the reference's track map, batched: inertial poses (X, Y, psi) -> curvilinear (s, ey, epsi)
// (Map.getLocalPosition, fnc/simulator/Track.py:191-290) and (s, epsi) -> psi (Map.getAngle, Track.py:312-349).  The forward half, Map.getGlobalPosition, is
// lmpc_global_position_kernel in lmpc_kernels.hip.h.  Included by lmpc_capi.hip only (the variant libraries carry no track kernel).
//
// Both kernels run one thread per point, LMPC_TRACK_NT threads per work-group, size_t indexing, the track table read from the lmpc_dev_params kernel argument as
// lmpc_global_position_kernel reads it -- or, in the TRK instantiations, from the point's own row of the track image (lmpc_track_set; lmpc_kernels.hip.h:
// lmpc_track_row) --; no LDS, no scratch.  The only loops are the walk over the track rows (bounded by track_rows) and the bounded lap wrap of s.
//
// getLocalPosition is a chain of branch tests on doubles (exact equality with a segment end point, |angle| <= pi / 2, sign(arc1) == sign(arc2), |arc1| >= |arc2|,
// |ey| <= max_ey).  Every function below switches contraction into FMAs off, as pid_control_law does, and evaluates products and sums in the order NumPy
// evaluates the reference's expressions: the tests then see the doubles NumPy sees, up to the few ulp by which ocml's atan2 / sin / cos differ from NumPy's.
#pragma once
#include <hip/hip_runtime.h>

#define LMPC_TRACK_NT 256                      // threads per work-group of the two kernels below: one thread per point
#define LMPC_TRACK_OFF 10000.0                 // s = ey = epsi of a point on no segment (Track.py:282-285)

// np.unwrap([a, b])[1]: b moved by a multiple of 2 pi when |b - a| >= pi.  NumPy: dd = b - a; ddmod = mod(dd + pi, 2 pi) - pi with the floored (Python) modulo;
// ddmod == -pi and dd > 0 -> +pi; correction ddmod - dd, dropped when |dd| < pi.  fmod is exact in IEEE arithmetic, on the device as in NumPy's C.
__device__ __forceinline__ double lmpc_unwrap2(double a, double b) {
#pragma clang fp contract(off)
    const double PI = 3.141592653589793, TWO_PI = 6.283185307179586;
    const double dd = b - a;
    double m = fmod(dd + PI, TWO_PI);
    if (m != 0.0) { if (m < 0.0) m += TWO_PI; } else m = 0.0;
    double ddmod = m - PI;
    if (ddmod == -PI && dd > 0.0) ddmod = PI;
    double corr = ddmod - dd;
    if (fabs(dd) < PI) corr = 0.0;
    return b + corr;
}

// computeAngle(point1, origin, point2), Track.py:356-365: atan2(det, dot) of v1 = point1 - origin, v2 = point2 - origin
__device__ __forceinline__ double lmpc_compute_angle(double p1x, double p1y, double ox, double oy, double p2x, double p2y) {
#pragma clang fp contract(off)
    const double v1x = p1x - ox, v1y = p1y - oy, v2x = p2x - ox, v2y = p2y - oy;
    const double dot = v1x * v2x + v1y * v2y;
    const double det = v1x * v2y - v1y * v2x;
    return atan2(det, dot);
}

// la.norm of a two-vector: sqrt(x . x)
__device__ __forceinline__ double lmpc_norm2(double x, double y) {
#pragma clang fp contract(off)
    return sqrt(x * x + y * y);
}

__device__ __forceinline__ double lmpc_sign(double a) { return (double)((a > 0.0) - (a < 0.0)); }     // np.sign of a number that is not NaN

// Map.getLocalPosition(x, y, psi) with halfWidth + slack = max_ey, branch for branch; the first completing row wins.  Returns the status word (0, or
// LMPC_ST_NO_SEGMENT with s = ey = epsi = 10000: no row completes, or an input is not finite).  Row i - 1 of row 0 is the last row (the reference's index -1).
template <class TK>
__device__ __forceinline__ int lmpc_local_position(const TK &p, double x, double y, double psi, double max_ey, double &s_out, double &ey_out, double &epsi_out) {
#pragma clang fp contract(off)
    const double PI = 3.141592653589793;
    s_out = LMPC_TRACK_OFF; ey_out = LMPC_TRACK_OFF; epsi_out = LMPC_TRACK_OFF;
    if (!(isfinite(x) && isfinite(y) && isfinite(psi))) return LMPC_ST_NO_SEGMENT;
    for (int i = 0; i < p.track_rows; i++) {
        const double *ti = p.track + i * 6, *tp = p.track + (i > 0 ? i - 1 : p.track_rows - 1) * 6;
        const double xf = ti[0], yf = ti[1], xs = tp[0], ys = tp[1], c0 = ti[3], len = ti[4], cur = ti[5], ang = tp[2];
        const bool at_start = lmpc_norm2(xs - x, ys - y) == 0.0, at_end = lmpc_norm2(xf - x, yf - y) == 0.0;
        if (cur == 0.0) {                                                                  // straight row
            const double epsi = lmpc_unwrap2(ang, psi) - ang;
            if (at_start) { s_out = c0; ey_out = 0.0; epsi_out = epsi; return 0; }
            if (at_end) { s_out = c0 + len; ey_out = 0.0; epsi_out = epsi; return 0; }
            if (fabs(lmpc_compute_angle(x, y, xs, ys, xf, yf)) <= PI / 2 && fabs(lmpc_compute_angle(x, y, xf, yf, xs, ys)) <= PI / 2) {
                const double nv = lmpc_norm2(x - xs, y - ys);
                const double angle = lmpc_compute_angle(xf, yf, xs, ys, x, y);
                const double s = nv * cos(angle) + c0, ey = nv * sin(angle);
                if (fabs(ey) <= max_ey) { s_out = s; ey_out = ey; epsi_out = epsi; return 0; }
            }
        } else {                                                                           // curved row
            const double r = 1 / cur, dir = r >= 0 ? 1.0 : -1.0, ar = fabs(r);
            const double cx = xs + ar * cos(ang + dir * PI / 2), cy = ys + ar * sin(ang + dir * PI / 2);
            if (at_start) { s_out = c0; ey_out = 0.0; epsi_out = lmpc_unwrap2(ang, psi) - ang; return 0; }
            if (at_end) { s_out = c0 + len; ey_out = 0.0; epsi_out = lmpc_unwrap2(ti[2], psi) - ti[2]; return 0; }
            const double arc1 = len * cur;
            const double arc2 = lmpc_compute_angle(xs, ys, cx, cy, x, y);
            if (arc2 == arc2 && lmpc_sign(arc1) == lmpc_sign(arc2) && fabs(arc1) >= fabs(arc2)) {
                const double s = fabs(arc2) * ar + c0;
                const double ey = -dir * (lmpc_norm2(x - cx, y - cy) - ar);
                const double a2 = ang + arc2;
                const double epsi = lmpc_unwrap2(a2, psi) - a2;
                if (fabs(ey) <= max_ey) { s_out = s; ey_out = ey; epsi_out = epsi; return 0; }
            }
        }
    }
    return LMPC_ST_NO_SEGMENT;
}

// Point e reads x[e in_stride], y[e in_stride], psi[e in_stride] and writes s[e out_stride], ey[e out_stride], epsi[e out_stride], status[e].  Stride 1: the three
// input and three output arrays of lmpc_local_position_batch.  Stride 6 with the pointers offset into T x B x 6 session logs: lmpc_state_from_global_batch, which
// also hands over copy_src / copy_dst -- the first three doubles of row e (vx, vy, wz) are then copied through unchanged.
// TRK (per-element tracks, lmpc_track_set): point e reads row (trkMod ? e % trkMod : e) of trk, trkStride doubles between rows (0: one row for all) -- trkMod = B for a
// T x B log, whose car b is on row b.
template <bool TRK>
__global__ void __launch_bounds__(LMPC_TRACK_NT) lmpc_local_position_kernel(lmpc_dev_params p, size_t n, const double *__restrict__ x, const double *__restrict__ y,
                                                                            const double *__restrict__ psi, size_t in_stride, double max_ey, double *__restrict__ s,
                                                                            double *__restrict__ ey, double *__restrict__ epsi, size_t out_stride, int *__restrict__ status,
                                                                            const double *__restrict__ copy_src, double *__restrict__ copy_dst,
                                                                            const double *__restrict__ trk, int trkStride, size_t trkMod) {
    const size_t e = (size_t)blockIdx.x * LMPC_TRACK_NT + threadIdx.x;
    if (e >= n) return;
    double so, eyo, epo;
    lmpc_track_row tr_ = {nullptr, 0, 0.0}; if constexpr (TRK) tr_ = track_row_at(trk, (size_t)trkStride, trkMod ? e % trkMod : e);
    const int st = lmpc_local_position(track_src<TRK>(p, tr_), x[e * in_stride], y[e * in_stride], psi[e * in_stride], max_ey, so, eyo, epo);
    if (copy_dst) { const double *cs = copy_src + e * in_stride; double *cd = copy_dst + e * out_stride; cd[0] = cs[0]; cd[1] = cs[1]; cd[2] = cs[2]; }
    s[e * out_stride] = so; ey[e * out_stride] = eyo; epsi[e * out_stride] = epo; status[e] = st;
}

// Map.getAngle(s, epsi), Track.py:312-349: the heading of a car at (s, epsi).  s is wrapped with the bounded loop of lmpc_global_position_kernel.  ang is 0 on
// row 0 (NOT the last row's psi: the reference's `if i > 0` here, against its index -1 in getLocalPosition).  status = LMPC_ST_NO_SEGMENT and psi = 0 where the
// reference raises (s on no row).
template <bool TRK>
__global__ void __launch_bounds__(LMPC_TRACK_NT) lmpc_track_angle_kernel(lmpc_dev_params p_, size_t n, const double *__restrict__ s_in, const double *__restrict__ epsi_in,
                                                                         double *__restrict__ psi_out, int *__restrict__ status, const double *__restrict__ trk, int trkStride) {
#pragma clang fp contract(off)
    const size_t e = (size_t)blockIdx.x * LMPC_TRACK_NT + threadIdx.x;
    if (e >= n) return;
    lmpc_track_row tr_ = {nullptr, 0, 0.0}; if constexpr (TRK) tr_ = track_row_at(trk, (size_t)trkStride, e);
    const auto &p = track_src<TRK>(p_, tr_);
    const double PI = 3.141592653589793;
    double s = s_in[e]; const double epsi = epsi_in[e];
    for (int lap = 0; lap < 4096 && s > p.TL; lap++) s = s - p.TL;                          // (`while s > TrackLength`, bounded: an infinite s must not hang the GPU)
    if (!(s <= p.TL)) s = -1.0;                                                               // -> on no segment
    int i = -1;
    for (int r = 0; r < p.track_rows; r++) { const double c0 = p.track[r * 6 + 3]; if (s >= c0 && s < c0 + p.track[r * 6 + 4]) { i = r; break; } }
    if (i < 0) { status[e] = LMPC_ST_NO_SEGMENT; psi_out[e] = 0.0; return; }
    const double *ti = p.track + i * 6;
    const double ang = i > 0 ? p.track[(i - 1) * 6 + 2] : 0.0;
    double psi;
    if (ti[5] == 0.0) psi = ang + epsi;
    else {
        const double r = 1 / ti[5];
        const double span = (s - ti[3]) / fabs(r);
        double a = ang + span * lmpc_sign(r);
        if (a < -PI) a = 2 * PI + a; else if (a > PI) a = a - 2 * PI;                       // wrap(), Track.py:367-375
        psi = a + epsi;
    }
    psi_out[e] = psi; status[e] = 0;
}

static inline unsigned lmpc_track_grid(size_t n) { return (unsigned)((n + LMPC_TRACK_NT - 1) / LMPC_TRACK_NT); }
