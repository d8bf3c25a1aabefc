// Rigid-body minimisation of a pose under the Vina-type interaction term `inter`, one launch: one workgroup owns a molecule
// for the whole minimisation and runs pair_sweep under VinaGradPolicy (vina_grad.h, unchanged) once per evaluation, in a
// loop; every decision is taken on the device by thread 0 and published through LDS.  The sweep's PairBatch::lig_x is the
// kernel's own coordinate output x_out: the coordinates of the pose under evaluation are written there before every sweep,
// and what the last sweep read is the result.  Pocket, codes and mol_int are constants of the launch.
//
// Pose: x0 the n input coordinates (read only), c0 their mean, s_i = x0_i - c0 (float64); the pose is (T, q), q a unit
// quaternion (w first), from (0, identity); x_i = float32((c0 + T) + R(q) s_i), formed in float64 and rounded once, always
// from x0: the result is a rigid image of the input up to one float32 rounding, whatever the number of steps.
// Scales: rho^2 = max(sum |s_i|^2 / n, 1), rho_max = max |s_i|.
//
// Iteration (vina._vina_minimize_host restates it; `step` L0, `tol`, `max_evals`).  An evaluation writes x(T, q), sweeps,
// and thread 0 reads back what `finish` stored as float32: E = inter (mol_out), F and M (mol_grad).
//   1. evaluate the input pose; E_start = E, L = L0
//   2. u = |F| + rho_max |M| / rho^2; not u > 0: stop, status 2 (no gradient: empty molecule or group, nothing typed)
//   3. L < tol: stop, status 1 (converged); max_evals evaluations made: stop, status 0; else with alpha = L / u the trial
//      T' = T - alpha F, q' = normalise(dq q), dq the rotation by -alpha M / rho^2 (about the centroid, world axes; no atom
//      moves more than L); evaluate; E' < E (float32, strict): take the trial, L = min(2 L, L0), go to 2; else L = L / 2, 3
//   4. on a stop after a rejected trial the accepted pose is evaluated once more (counted, the one evaluation allowed beyond
//      max_evals), so that every output row describes the returned pose.
// A molecule with a coordinate that is not finite: status 3, its x_out rows are the input's bits, NaN in every other float
// it owns, the flag.
//
// Control flow is workgroup-uniform: `go` is one LDS word that thread 0 writes and every thread reads after a barrier, so
// every thread enters pair_sweep the same number of times, at most max_evals + 1 (the loop's own bound).  The state of the
// iteration lives in LDS, not in registers held across the sweep.  No atomics; sums in a fixed order: bitwise reproducible
// and independent of the rest of the batch.
#pragma once
#include "vina_grad.h"

namespace dsbdd {

constexpr int kVinaMolPose = 8;      // floats per molecule: T (3), q (4, w first), rho^2
constexpr int kVinaMolMin = 4;       // floats per molecule: E_start, E_final, the last accepted L (0 if none), u at the returned pose
constexpr int kVinaMolStat = 4;      // ints per molecule: status, evaluations, accepted steps, 0
constexpr int kVinaMaxEvals = 4096;
enum VinaMinStatus { kVinaMinBudget = 0, kVinaMinConverged, kVinaMinNoGradient, kVinaMinNonfinite };

struct VinaMinArgs {
  VinaGradArgs grad;       // what vina_grad_kernel takes; grad.score.pairs.lig_x is x_out
  const float* x0;         // [N][3] the input pose
  float step, tol;
  int max_evals;           // in [1, kVinaMaxEvals]
  float* x_out;            // [N][3]
  float* mol_pose;         // [B][kVinaMolPose]
  float* mol_min;          // [B][kVinaMolMin]
  int* mol_stat;           // [B][kVinaMolStat]
};

struct VinaMinState {      // in LDS; thread 0 alone reads and writes everything but `frame` and `go`
  double T[3], q[4];       // the accepted pose
  double Tt[3], qt[4];     // the trial under evaluation
  double F[3], M[3], u;    // at the accepted pose, from the stored float32 values
  double L, last_L;
  float E, E_start;
  int evals, accepted, status, phase, rejected;
  double frame[12];        // published: R(q) row-major (9), c0 + T (3) of the pose to evaluate
  int go;                  // published: 1 = evaluate `frame`, 0 = done
};
enum VinaMinPhase { kVinaMinFirst = 0, kVinaMinTrial, kVinaMinFinal };

// R(q) and c0 + T of a pose, to `frame`
__device__ inline void vina_min_frame(double* frame, const double* c0, const double* T, const double* q) {
  const double w = q[0], x = q[1], y = q[2], z = q[3];
  frame[0] = 1.0 - 2.0 * (y * y + z * z); frame[1] = 2.0 * (x * y - w * z); frame[2] = 2.0 * (x * z + w * y);
  frame[3] = 2.0 * (x * y + w * z); frame[4] = 1.0 - 2.0 * (x * x + z * z); frame[5] = 2.0 * (y * z - w * x);
  frame[6] = 2.0 * (x * z - w * y); frame[7] = 2.0 * (y * z + w * x); frame[8] = 1.0 - 2.0 * (x * x + y * y);
  for (int k = 0; k < 3; ++k) frame[9 + k] = c0[k] + T[k];
}

// three sums and a maximum over the workgroup, lanes by butterfly, waves in wave order; every thread gets them
__device__ inline void vina_min_reduce(double* v, double& top, double (*red)[4]) {
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  for (int o = 32; o; o >>= 1) {
    for (int k = 0; k < 3; ++k) v[k] += __shfl_xor(v[k], o);
    top = fmax(top, __shfl_xor(top, o));
  }
  if (lane == 0) {
    for (int k = 0; k < 3; ++k) red[wave][k] = v[k];
    red[wave][3] = top;
  }
  __syncthreads();
  for (int k = 0; k < 3; ++k) v[k] = 0.0;
  top = 0.0;
  for (int w = 0; w < kThreads / 64; ++w) {
    for (int k = 0; k < 3; ++k) v[k] += red[w][k];
    top = fmax(top, red[w][3]);
  }
  __syncthreads();                                                  // red may be written again
}

// thread 0, after a sweep: read the stored rows, take the decision, publish the next pose or the end
__device__ inline void vina_min_decide(const VinaMinArgs& a, int b, VinaMinState& st, const double* c0, double rho2, double rho_max) {
  const float* mo = a.grad.score.mol_out + (size_t)kVinaMolOut * b;
  const float* mg = a.grad.mol_grad + (size_t)kVinaMolGrad * b;
  const float E1 = mo[5];
  ++st.evals;
  if (st.phase == kVinaMinFinal) {                                  // the accepted pose, evaluated again: its rows stand
    st.go = 0;
    return;
  }
  bool moved = false;
  if (st.phase == kVinaMinFirst) {
    st.E = st.E_start = E1;
    st.L = (double)a.step;
    moved = true;
  } else if (E1 < st.E) {
    for (int k = 0; k < 3; ++k) st.T[k] = st.Tt[k];
    for (int k = 0; k < 4; ++k) st.q[k] = st.qt[k];
    st.E = E1;
    st.last_L = st.L;
    st.L = fmin(2.0 * st.L, (double)a.step);
    ++st.accepted;
    st.rejected = 0;
    moved = true;
  } else {
    st.L *= 0.5;
    st.rejected = 1;
  }
  bool stop = false;
  if (moved) {
    for (int k = 0; k < 3; ++k) {
      st.F[k] = (double)mg[k];
      st.M[k] = (double)mg[3 + k];
    }
    const double f = sqrt((st.F[0] * st.F[0] + st.F[1] * st.F[1]) + st.F[2] * st.F[2]);
    const double m = sqrt((st.M[0] * st.M[0] + st.M[1] * st.M[1]) + st.M[2] * st.M[2]);
    st.u = f + rho_max * m / rho2;
    if (!(st.u > 0.0)) {
      st.status = kVinaMinNoGradient;
      stop = true;
    }
  }
  if (!stop) {
    if (st.L < (double)a.tol) {
      st.status = kVinaMinConverged;
      stop = true;
    } else if (st.evals >= a.max_evals) {
      st.status = kVinaMinBudget;
      stop = true;
    }
  }
  if (stop) {
    if (st.rejected) {                                              // x_out and the rows hold the rejected trial
      vina_min_frame(st.frame, c0, st.T, st.q);
      st.phase = kVinaMinFinal;
      st.go = 1;
    } else {
      st.go = 0;
    }
    return;
  }
  const double alpha = st.L / st.u;
  double th[3];
  for (int k = 0; k < 3; ++k) {
    st.Tt[k] = st.T[k] - alpha * st.F[k];
    th[k] = -(alpha * st.M[k]) / rho2;
  }
  const double angle = sqrt((th[0] * th[0] + th[1] * th[1]) + th[2] * th[2]);
  double dq[4] = {1.0, 0.0, 0.0, 0.0};
  if (angle > 0.0) {
    const double h = 0.5 * angle, s = sin(h) / angle;
    dq[0] = cos(h);
    for (int k = 0; k < 3; ++k) dq[1 + k] = s * th[k];
  }
  const double* q = st.q;
  double r[4] = {dq[0] * q[0] - dq[1] * q[1] - dq[2] * q[2] - dq[3] * q[3],
                 dq[0] * q[1] + dq[1] * q[0] + dq[2] * q[3] - dq[3] * q[2],
                 dq[0] * q[2] - dq[1] * q[3] + dq[2] * q[0] + dq[3] * q[1],
                 dq[0] * q[3] + dq[1] * q[2] - dq[2] * q[1] + dq[3] * q[0]};
  const double norm = sqrt((r[0] * r[0] + r[1] * r[1]) + (r[2] * r[2] + r[3] * r[3]));
  for (int k = 0; k < 4; ++k) st.qt[k] = r[k] / norm;
  vina_min_frame(st.frame, c0, st.Tt, st.qt);
  st.phase = kVinaMinTrial;
  st.go = 1;
}

__global__ __launch_bounds__(kThreads) void vina_minimize_kernel(VinaMinArgs a) {
  __shared__ VinaGradPolicy::Total part[kThreads / 64];
  __shared__ double red[kThreads / 64][4];
  __shared__ VinaMinState st;
  const int b = blockIdx.x, tid = threadIdx.x;
  const PairRows rows = pair_rows(a.grad.score.pairs, b);
  const int n = rows.n;
  const float* x0 = a.x0 + 3 * (size_t)rows.lo;
  float* x = a.x_out + 3 * (size_t)rows.lo;
  VinaScoreArgs in = a.grad.score;                                  // the scan for coordinates that are not finite reads the input
  in.pairs.lig_x = a.x0;
  if (vina_nonfinite(in, rows, b)) {
    const float nan = __builtin_nanf("");
    for (int k = tid; k < 3 * n; k += kThreads) {
      x[k] = x0[k];
      a.grad.atom_grad[3 * (size_t)rows.lo + k] = nan;
    }
    if (tid < kVinaMolGrad) a.grad.mol_grad[(size_t)kVinaMolGrad * b + tid] = nan;
    if (tid < kVinaMolPose) a.mol_pose[(size_t)kVinaMolPose * b + tid] = nan;
    if (tid < kVinaMolMin) a.mol_min[(size_t)kVinaMolMin * b + tid] = nan;
    if (tid < kVinaMolStat) a.mol_stat[(size_t)kVinaMolStat * b + tid] = tid == 0 ? (int)kVinaMinNonfinite : 0;
    return;
  }
  // c0, then rho^2 and rho_max: every thread holds them
  double c0[3] = {0, 0, 0}, none = 0.0;
  for (int i = tid; i < n; i += kThreads)
    for (int k = 0; k < 3; ++k) c0[k] += (double)x0[3 * (size_t)i + k];
  vina_min_reduce(c0, none, red);
  if (n > 0)
    for (int k = 0; k < 3; ++k) c0[k] /= (double)n;
  double sq[3] = {0, 0, 0}, top = 0.0;
  for (int i = tid; i < n; i += kThreads) {
    double s2 = 0.0;
    for (int k = 0; k < 3; ++k) {
      const double s = (double)x0[3 * (size_t)i + k] - c0[k];
      s2 += s * s;
    }
    sq[0] += s2;
    top = fmax(top, s2);
  }
  vina_min_reduce(sq, top, red);
  const double rho2 = n > 0 ? fmax(sq[0] / (double)n, 1.0) : 1.0, rho_max = sqrt(top);
  if (tid == 0) {
    for (int k = 0; k < 3; ++k) st.T[k] = st.Tt[k] = 0.0;
    for (int k = 0; k < 4; ++k) st.q[k] = st.qt[k] = k == 0 ? 1.0 : 0.0;
    for (int k = 0; k < 3; ++k) st.F[k] = st.M[k] = 0.0;
    st.u = st.L = st.last_L = 0.0;
    st.E = st.E_start = 0.0f;
    st.evals = st.accepted = st.rejected = 0;
    st.status = kVinaMinBudget;
    st.phase = kVinaMinFirst;
    vina_min_frame(st.frame, c0, st.T, st.q);
    st.go = 1;
  }
  VinaGradPolicy pol{a.grad, {a.grad.score, nullptr}, part};
  for (int sweep = 0; sweep <= a.max_evals; ++sweep) {              // at most max_evals + 1 sweeps, whatever thread 0 decides
    __syncthreads();                                                // thread 0's frame and `go`; the sweep before is over
    if (!__builtin_amdgcn_readfirstlane(st.go)) break;              // one LDS word, the same in every thread
    double f[12];
    for (int k = 0; k < 12; ++k) f[k] = st.frame[k];
    for (int i = tid; i < n; i += kThreads) {
      double s[3];
      for (int k = 0; k < 3; ++k) s[k] = (double)x0[3 * (size_t)i + k] - c0[k];
      for (int k = 0; k < 3; ++k)
        x[3 * (size_t)i + k] = (float)(f[9 + k] + ((f[3 * k] * s[0] + f[3 * k + 1] * s[1]) + f[3 * k + 2] * s[2]));
    }
    __syncthreads();                                                // the coordinates, before any wave's sweep reads them
    pair_sweep(a.grad.score.pairs, rows, pol);
    if (tid == 0) vina_min_decide(a, b, st, c0, rho2, rho_max);     // reads the rows it stored itself in `finish`
  }
  if (tid == 0) {
    float* pose = a.mol_pose + (size_t)kVinaMolPose * b;
    for (int k = 0; k < 3; ++k) pose[k] = (float)st.T[k];
    for (int k = 0; k < 4; ++k) pose[3 + k] = (float)st.q[k];
    pose[7] = (float)rho2;
    float* mn = a.mol_min + (size_t)kVinaMolMin * b;
    mn[0] = st.E_start; mn[1] = st.E; mn[2] = (float)st.last_L; mn[3] = (float)st.u;
    int* stat = a.mol_stat + (size_t)kVinaMolStat * b;
    stat[0] = st.status; stat[1] = st.evals; stat[2] = st.accepted; stat[3] = 0;
  }
}

}  // namespace dsbdd
