// pwc_track.hip -- point tracking: query points carried through the consecutive flows of a sequence, a position and a status per
// point and frame (gfx950; C ABI in include/pwc_hip.h, "point tracking"; semantics and launch plan in DESIGN.md 17).
//
//   pwc_track_points_f32    tracks (T + 1, P, 2) float32 and status (T + 1, P) bytes from the flows t -> t + 1 (and, for the
//                           forward-backward check and the walk towards frame 0, the flows t + 1 -> t) of T + 1 frames
//
// One step carries a point in state (x, y) float32, status s, across one flow F (the step flow), checked against G (the flow
// of the opposite direction between the same two frames, where given).  Every operation is an IEEE double + - x, a floor or a
// comparison in the order written in track_step / track_sample below -- no fused multiply-add is formed anywhere in this file
// (the pragma below) -- so tests/track_ref.py restates it in numpy bit for bit.
//   terminal s (LEFT, UNKNOWN, OCCLUDED with stop_on_occlusion, any byte that is no status code): position and status repeat.
//   A  the point is not in [0, W - 1] x [0, H - 1] (a NaN fails)                           -> LEFT, position kept
//   B  one of the four clamped corners around it is masked out in F's mask or holds a component that is not finite or beyond
//      1e9 in magnitude (flow_io.flow_valid's rule) -- all four whatever their weight     -> UNKNOWN, position kept
//      S = the bilinear sample of F (pwc_fb_valid_u8's, word for word), r = q + S
//   C  r is not in the frame                                                              -> LEFT, position kept
//   D  (G given) a bad corner of G around r                                               -> UNKNOWN, position kept
//      b = the sample of G at r; alpha1 ((S.S) + (b.b)) + alpha2 - |S + b|^2 >= 0 fails   -> OCCLUDED, position (float)r
//      else VISIBLE, position (float)r: rounded once.
// Every decision is a branch: a point that fails A reads no flow, one that fails B no check flow, a masked corner's flow is not
// loaded -- a NaN in a place the rule excludes reaches nothing.  The in-frame tests are what keep the corner reads inside the
// frame: 0 <= x0 <= x1 <= W - 1 and the same in y follow from them.
// One lane per point walks its slices (the chain in t is dependent; the parallelism is over P): from its start slice up to T,
// and with direction BOTH down to 0 with the roles of the two flows and masks swapped.  The outputs are time-major, so the
// lanes of a wave store neighbouring records of one slice.  No LDS, no atomics, no workspace; 64-bit indices into (T + 1) P.
// Flows at any channel stride >= 2: where every float pointer of a call is on an 8-byte boundary and every channel stride is
// even a record's two floats are one 8-byte access, else two 4-byte ones -- the values, and so every bit, are the same
// (flow_record.h).
#include "flow_record.h"

#pragma clang fp contract(off)

struct TrackArgs {
    const float* fw;          // [T][H][W] records of fw_cs floats, 2 used: the flows t -> t + 1
    const float* bw;          // the flows t + 1 -> t, or null
    const uint8_t* vfw;       // [T][H][W], null: every pixel
    const uint8_t* vbw;
    const float* points;      // [P][2]
    const int* start;         // [P], null: 0
    const uint8_t* status_in; // [P], null: every point starts fresh
    float* tracks;            // [T + 1][P][2]
    uint8_t* status;          // [T + 1][P]
    int fw_cs, bw_cs;
    int T, H, W, P;
    int both, stop;
    float alpha1, alpha2;
};

__device__ __forceinline__ bool track_inside(double qx, double qy, int H, int W) {
    return qx >= 0.0 && qx <= (double)(W - 1) && qy >= 0.0 && qy <= (double)(H - 1);
}

// The bilinear sample of one frame's flow f (mask m or null) at a point INSIDE the frame; false where a corner is masked out or
// unknown, and then s0, s1 are not written.
template <bool VEC>
__device__ __forceinline__ bool track_sample(const float* f, int cs, const uint8_t* m, int H, int W, double qx, double qy,
                                             double& s0, double& s1) {
    const PwcBilinearF64 bl = pwc_bilinear_f64(qx, qy, H, W);
    const double wx = bl.wx1, wy = bl.wy1;
    const size_t o00 = bl.o00, o01 = bl.o01, o10 = bl.o10, o11 = bl.o11;
    if (m && !(m[o00] && m[o01] && m[o10] && m[o11])) return false;
    float c00[2], c01[2], c10[2], c11[2];
    pwc_flow_load2<VEC>(f + o00 * cs, c00[0], c00[1]);
    pwc_flow_load2<VEC>(f + o01 * cs, c01[0], c01[1]);
    pwc_flow_load2<VEC>(f + o10 * cs, c10[0], c10[1]);
    pwc_flow_load2<VEC>(f + o11 * cs, c11[0], c11[1]);
    if (!(pwc_flow_known(c00[0], c00[1]) && pwc_flow_known(c01[0], c01[1]) && pwc_flow_known(c10[0], c10[1]) &&
          pwc_flow_known(c11[0], c11[1])))
        return false;
    const double ux = bl.wx0, uy = bl.wy0;
    s0 = (uy * ((ux * (double)c00[0]) + (wx * (double)c01[0]))) + (wy * ((ux * (double)c10[0]) + (wx * (double)c11[0])));
    s1 = (uy * ((ux * (double)c00[1]) + (wx * (double)c01[1]))) + (wy * ((ux * (double)c10[1]) + (wx * (double)c11[1])));
    return true;
}

// One step across the frame pair whose step flow is F and whose check flow is G (null: no check).
template <bool VEC>
__device__ __forceinline__ void track_step(const TrackArgs& a, const float* F, int f_cs, const uint8_t* Fm, const float* G, int g_cs,
                                           const uint8_t* Gm, float& x, float& y, int& s) {
    if (!(s == PWC_TRACK_VISIBLE || (s == PWC_TRACK_OCCLUDED && !a.stop))) return;
    const double qx = (double)x, qy = (double)y;
    if (!track_inside(qx, qy, a.H, a.W)) { s = PWC_TRACK_LEFT; return; }
    double S0, S1;
    if (!track_sample<VEC>(F, f_cs, Fm, a.H, a.W, qx, qy, S0, S1)) { s = PWC_TRACK_UNKNOWN; return; }
    const double rx = qx + S0, ry = qy + S1;
    if (!track_inside(rx, ry, a.H, a.W)) { s = PWC_TRACK_LEFT; return; }
    int ns = PWC_TRACK_VISIBLE;
    if (G) {
        double b0, b1;
        if (!track_sample<VEC>(G, g_cs, Gm, a.H, a.W, rx, ry, b0, b1)) { s = PWC_TRACK_UNKNOWN; return; }
        const double d0 = S0 + b0, d1 = S1 + b1;
        const double bound = ((double)a.alpha1 * (((S0 * S0) + (S1 * S1)) + ((b0 * b0) + (b1 * b1)))) + (double)a.alpha2;
        const double margin = bound - ((d0 * d0) + (d1 * d1));
        if (!(margin >= 0.0)) ns = PWC_TRACK_OCCLUDED;
    }
    s = ns;
    x = (float)rx;
    y = (float)ry;
}

// One lane per point.
template <bool VEC>
__global__ __launch_bounds__(256) void track_points_kernel(const TrackArgs a) {
    const size_t frame = (size_t)a.H * a.W;
    const long P = a.P;
    for (long p = blockIdx.x * 256L + threadIdx.x; p < P; p += (long)gridDim.x * 256) {
        float px, py;
        pwc_flow_load2<VEC>(a.points + 2 * p, px, py);
        int s0 = a.start ? a.start[p] : 0;
        int st = a.status_in ? (int)a.status_in[p] : PWC_TRACK_UNSEEN;
        if (st != PWC_TRACK_UNSEEN) {
            s0 = 0;                                                        // the streaming form: the state of slice 0 is given
        } else if (s0 < 0 || s0 > a.T) {                                   // not in this call
            for (long t = 0; t <= a.T; ++t) {
                pwc_flow_store2<VEC>(a.tracks + 2 * (t * P + p), px, py);
                a.status[t * P + p] = PWC_TRACK_UNSEEN;
            }
            continue;
        } else {
            st = track_inside((double)px, (double)py, a.H, a.W) ? PWC_TRACK_VISIBLE : PWC_TRACK_LEFT;
        }
        pwc_flow_store2<VEC>(a.tracks + 2 * ((long)s0 * P + p), px, py);
        a.status[(long)s0 * P + p] = (uint8_t)st;
        float x = px, y = py;
        int s = st;
        for (long t = s0; t < a.T; ++t) {
            track_step<VEC>(a, a.fw + t * frame * a.fw_cs, a.fw_cs, a.vfw ? a.vfw + t * frame : nullptr,
                            a.bw ? a.bw + t * frame * a.bw_cs : nullptr, a.bw_cs, a.vbw ? a.vbw + t * frame : nullptr, x, y, s);
            pwc_flow_store2<VEC>(a.tracks + 2 * ((t + 1) * P + p), x, y);
            a.status[(t + 1) * P + p] = (uint8_t)s;
        }
        x = px; y = py; s = st;
        for (long t = s0; t > 0; --t) {
            if (a.both) {                                                  // t -> t - 1: flows_bw[t - 1] steps, flows_fw[t - 1] checks
                track_step<VEC>(a, a.bw + (t - 1) * frame * a.bw_cs, a.bw_cs, a.vbw ? a.vbw + (t - 1) * frame : nullptr,
                                a.fw + (t - 1) * frame * a.fw_cs, a.fw_cs, a.vfw ? a.vfw + (t - 1) * frame : nullptr, x, y, s);
            } else {
                s = PWC_TRACK_UNSEEN;
            }
            pwc_flow_store2<VEC>(a.tracks + 2 * ((t - 1) * P + p), x, y);
            a.status[(t - 1) * P + p] = (uint8_t)s;
        }
    }
}

// ---------------------------------------------------------------- host
extern "C" int pwc_track_points_f32(const float* flows_fw, int fw_cs, const float* flows_bw, int bw_cs, const uint8_t* valids_fw,
                                    const uint8_t* valids_bw, int T, int H, int W, const float* points, const int32_t* start,
                                    const uint8_t* status_in, int P, int direction, float alpha1, float alpha2,
                                    int stop_on_occlusion, float* tracks, uint8_t* status, pwc_stream_t stream) {
    if (!flows_fw || !points || !tracks || !status || T < 1 || H < 1 || W < 1 || P < 1 || fw_cs < 2 || (flows_bw && bw_cs < 2))
        return PWC_EINVAL;
    if (direction != PWC_TRACK_FORWARD && direction != PWC_TRACK_BOTH) return PWC_EINVAL;
    if (direction == PWC_TRACK_BOTH && !flows_bw) return PWC_EINVAL;
    if (flows_bw && (!(alpha1 >= 0.f) || !(alpha2 >= 0.f))) return PWC_EINVAL;     // (a NaN fails both)
    // (float)rx with rx <= W - 1 stays inside the frame only while W - 1 is a float32: W <= 2^24
    if (H > (1 << 24) || W > (1 << 24) || (long)H * W >= (1L << 31) || T > 65535) return PWC_ERANGE;
    if (pwc_off(flows_fw, 3u) || (flows_bw && pwc_off(flows_bw, 3u)) || pwc_off(points, 3u) || pwc_off(tracks, 3u) ||
        (start && pwc_off(start, 3u)))
        return PWC_EALIGN;
    TrackArgs a = {};
    a.fw = flows_fw; a.bw = flows_bw; a.vfw = valids_fw; a.vbw = flows_bw ? valids_bw : nullptr;
    a.points = points; a.start = start; a.status_in = status_in; a.tracks = tracks; a.status = status;
    a.fw_cs = fw_cs; a.bw_cs = flows_bw ? bw_cs : 2; a.T = T; a.H = H; a.W = W; a.P = P;
    a.both = direction == PWC_TRACK_BOTH ? 1 : 0;
    a.stop = stop_on_occlusion ? 1 : 0;
    a.alpha1 = alpha1; a.alpha2 = alpha2;
    const bool vec = pwc_flow_vec(a.fw_cs | a.bw_cs, {flows_fw, flows_bw, points, tracks});
    const dim3 grid = pwc_flat_grid(P);
    if (vec) hipLaunchKernelGGL(track_points_kernel<true>, grid, dim3(256), 0, (hipStream_t)stream, a);
    else hipLaunchKernelGGL(track_points_kernel<false>, grid, dim3(256), 0, (hipStream_t)stream, a);
    return pwc_launch_status();
}
