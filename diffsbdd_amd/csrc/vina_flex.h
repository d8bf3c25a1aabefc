// Flexible minimisation of a pose under E = inter + intra of the Vina-type score, one launch after the typing and the
// torsion tree: the structure of vina_minimize_kernel (vina_minimize.h) with the rotatable bonds of vina_torsion.h as
// further degrees of freedom and the intramolecular term of vina_intra.h in the objective.  One workgroup owns a molecule
// for the whole minimisation; per evaluation it writes the coordinates of the pose to x_out, runs pair_sweep under
// VinaGradPolicy (the pocket) and under VinaIntraPolicy (the molecule itself), and thread 0 decides from the rows the two
// `finish` calls stored.  Control flow is workgroup-uniform (every branch that holds a barrier tests LDS words thread 0
// published before a barrier), the sweep loop is bounded by max_evals + 1 whatever thread 0 decides, the state lives in
// LDS, there are no atomics, and every index read from device memory is range-checked before it is used: the rows as
// pair_rows checks them, the kept count clamped to [0, kVinaMaxTorsions], a rotor whose ends are not two different atoms
// of the molecule is dropped (the molecule relaxes with the others), side bits at or above n are cleared, and a molecule
// longer than 128 atoms has no rotor.
//
// Degrees of freedom: (t, q, theta_1 ... theta_K), K <= 32 the rotors that passed the check, in list order; `dofs` bit 0 =
// the rigid body (t, q), bit 1 = the torsions; a block that is switched off is never stepped (without bit 1, K = 0).
//
// Coordinates, always from the input x0, in float64, rounded once:  y = x0;  for k in list order with theta_k != 0 and an
// axis of non-zero length: the atoms of S_k turn by theta_k about the line from y[p_k] through y[m_k] as it stands then
// (v = y_i - y[m_k], a the unit axis: y_i = y[m_k] + v cos + (a x v) sin + a (a . v)(1 - cos));  x_i = float32(t + R(q) y_i).
// The start is theta = 0, t = 0, q = identity: x = x0 bit for bit.  A rotation moves a side rigidly and the atoms of an
// axis are either both inside a side or both outside (the S_k are nested or disjoint, vina_torsion.h), so bond lengths,
// angles and every distance inside a rigid piece are the input's up to the float64 arithmetic and one float32 rounding,
// after any number of steps; and for the same reason the geometry does not depend on the list order in real arithmetic:
// turning an outer side carries every inner axis along with its side, turning an inner side leaves the outer axis alone.
//
// Objective: E = (double)inter32 + (double)intra32 of the rows the two sweeps stored; trials are compared with strict <.
//
// Gradient, at an accepted pose x (the float32 coordinates in x_out), c their mean:  F and M are the float32 mol_grad rows of
// the pocket sweep (net force and moment about c; intramolecular forces are internal and add nothing to either);
// tau_k = a_k . sum_{i in S_k} (x_i - x_{m_k}) x (g_i^inter + g_i^intra), a_k the unit vector from x_{p_k} to x_{m_k} (tau_k = 0
// if the ends coincide), the float32 gradient rows converted and summed in float64, lanes by butterfly.
//
// Step: at every accepted pose rho^2 = max(mean |x_i - c|^2, 1), rho_max = max |x_i - c|, and per rotor r_k = max over S_k
// of the distance to axis k, rho_k^2 = max(mean over S_k of that distance squared, 1);  u = |F| + rho_max |M| / rho^2 +
// sum_k r_k |tau_k| / rho_k^2 (a switched-off block left out);  alpha = L / u;  the trial: the rigid motion "rotate by
// -alpha M / rho^2 about c, translate by -alpha F", i.e. q' = normalise(dq q), t' = c + R(dq)(t - c) - alpha F, and
// theta_k' = theta_k - alpha tau_k / rho_k^2.
// No atom moves more than L in a trial (up to roundings).  Apply the rigid motion to the accepted pose first: an atom at most
// rho_max from c moves at most alpha |F| + rho_max alpha |M| / rho^2.  Then turn the rotors, outermost sides first, each by its
// change of angle: when rotor k turns, its side still has the shape of the accepted pose (only sides outside it have turned,
// carrying it and its axis rigidly), so an atom of S_k moves at most r_k alpha |tau_k| / rho_k^2 and no other atom moves.
// By the order independence above the result is the trial pose, and by the triangle inequality every atom has moved at
// most alpha u = L.
//
// Accept, halve and double back, tol, max_evals, the evaluation of the accepted pose once more after a stop on a rejected
// trial, and the statuses are those of vina_minimize.h (status 2: u is not > 0).  A molecule with a coordinate that is not
// finite: status 3, x_out the input's bits, NaN in every other float it owns, both flags.
#pragma once
#include "vina_intra.h"
#include "vina_minimize.h"

namespace dsbdd {

constexpr int kVinaMolFlex = 8;     // floats per molecule: inter at the start, at the end, the last accepted L (0 if none), u at the
                                    // returned pose, intra at the start, at the end, E at the start, at the end
constexpr int kVinaDofRigid = 1, kVinaDofTorsions = 2;

struct VinaFlexArgs {
  VinaMinArgs min;         // what vina_minimize_kernel takes; min.mol_min is [B][kVinaMolFlex]
  VinaIntraArgs intra;     // what vina_intra_kernel takes, its coordinates x_out
  const int* tor_int;      // what vina_torsion_kernel wrote
  const int* tor_end;
  const int* tor_side;
  int dofs;
  float* theta;            // [B][kVinaMaxTorsions] at the returned pose; 0 for a slot that is not a kept, valid rotor
  float* tau;              // [B][kVinaMaxTorsions]
};

struct VinaFlexState {     // in LDS; thread 0 writes, everything the workgroup reads is read after a barrier
  double t[3], q[4], th[kVinaMaxTorsions];          // the accepted pose
  double tt[3], qt[4], tht[kVinaMaxTorsions];       // the pose under evaluation
  double F[3], M[3], c[3], rho2, rho_max;           // at the accepted pose
  double tau[kVinaMaxTorsions], reach[kVinaMaxTorsions], rho2k[kVinaMaxTorsions];     // written by lane 0 of the rotor's wave
  double u, L, last_L, E, E_start;
  float inter_start, intra_start;
  int evals, accepted, status, phase, rejected;
  int K, p[kVinaMaxTorsions], m[kVinaMaxTorsions], slot[kVinaMaxTorsions];
  VinaMask side[kVinaMaxTorsions];
  int go, moved;
};

// thread 0, after the two sweeps: the energy of the pose evaluated, and whether it becomes the accepted pose
__device__ inline void vina_flex_judge(const VinaFlexArgs& a, int b, VinaFlexState& st) {
  const float inter = a.min.grad.score.mol_out[(size_t)kVinaMolOut * b + 5];
  const float intra = a.intra.out.score.mol_out[(size_t)kVinaMolOut * b + 5];
  const double E1 = (double)inter + (double)intra;
  ++st.evals;
  st.moved = 0;
  if (st.phase == kVinaMinFinal) return;
  if (st.phase == kVinaMinFirst) {
    st.E = st.E_start = E1;
    st.inter_start = inter;
    st.intra_start = intra;
    st.L = (double)a.min.step;
    st.moved = 1;
  } else if (E1 < st.E) {
    for (int k = 0; k < 3; ++k) st.t[k] = st.tt[k];
    for (int k = 0; k < 4; ++k) st.q[k] = st.qt[k];
    for (int k = 0; k < st.K; ++k) st.th[k] = st.tht[k];
    st.E = E1;
    st.last_L = st.L;
    st.L = fmin(2.0 * st.L, (double)a.min.step);
    ++st.accepted;
    st.rejected = 0;
    st.moved = 1;
  } else {
    st.L *= 0.5;
    st.rejected = 1;
  }
}

// thread 0, after the geometry of a newly accepted pose: stop, or publish the next trial
__device__ inline void vina_flex_step(const VinaFlexArgs& a, int b, VinaFlexState& st) {
  if (st.phase == kVinaMinFinal) {                                  // the accepted pose, evaluated again: its rows stand
    st.go = 0;
    return;
  }
  const bool rigid = (a.dofs & kVinaDofRigid) != 0;
  bool stop = false;
  if (st.moved) {
    const float* mg = a.min.grad.mol_grad + (size_t)kVinaMolGrad * b;
    for (int k = 0; k < 3; ++k) {
      st.F[k] = (double)mg[k];
      st.M[k] = (double)mg[3 + k];
    }
    double u = 0.0;
    if (rigid) {
      const double f = sqrt((st.F[0] * st.F[0] + st.F[1] * st.F[1]) + st.F[2] * st.F[2]);
      const double m = sqrt((st.M[0] * st.M[0] + st.M[1] * st.M[1]) + st.M[2] * st.M[2]);
      u = f + st.rho_max * m / st.rho2;
    }
    for (int k = 0; k < st.K; ++k) u += st.reach[k] * fabs(st.tau[k]) / st.rho2k[k];
    st.u = u;
    if (!(u > 0.0)) {
      st.status = kVinaMinNoGradient;
      stop = true;
    }
  }
  if (!stop) {
    if (st.L < (double)a.min.tol) {
      st.status = kVinaMinConverged;
      stop = true;
    } else if (st.evals >= a.min.max_evals) {
      st.status = kVinaMinBudget;
      stop = true;
    }
  }
  if (stop) {
    if (st.rejected) {                                              // x_out and the rows hold the rejected trial
      for (int k = 0; k < 3; ++k) st.tt[k] = st.t[k];
      for (int k = 0; k < 4; ++k) st.qt[k] = st.q[k];
      for (int k = 0; k < st.K; ++k) st.tht[k] = st.th[k];
      st.phase = kVinaMinFinal;
      st.go = 1;
    } else {
      st.go = 0;
    }
    return;
  }
  const double alpha = st.L / st.u;
  for (int k = 0; k < 3; ++k) st.tt[k] = st.t[k];
  for (int k = 0; k < 4; ++k) st.qt[k] = st.q[k];
  if (rigid) {
    double th[3];
    for (int k = 0; k < 3; ++k) th[k] = -(alpha * st.M[k]) / st.rho2;
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
    double f[12], s[3];
    const double zero[3] = {0.0, 0.0, 0.0};
    vina_min_frame(f, zero, zero, dq);                              // R(dq)
    for (int k = 0; k < 3; ++k) s[k] = st.t[k] - st.c[k];
    for (int k = 0; k < 3; ++k)
      st.tt[k] = (st.c[k] + ((f[3 * k] * s[0] + f[3 * k + 1] * s[1]) + f[3 * k + 2] * s[2])) - alpha * st.F[k];
  }
  for (int k = 0; k < st.K; ++k) st.tht[k] = st.th[k] - (alpha * st.tau[k]) / st.rho2k[k];
  st.phase = kVinaMinTrial;
  st.go = 1;
}

__global__ __launch_bounds__(kThreads) void vina_flex_kernel(VinaFlexArgs a) {
  __shared__ VinaGradPolicy::Total part[kThreads / 64];
  __shared__ VinaIntraPolicy::Total intra_part[kThreads / 64];
  __shared__ double red[kThreads / 64][4];
  __shared__ double y[kMolMaxAtoms][3];
  __shared__ VinaFlexState st;
  const int b = blockIdx.x, tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const PairRows rows = pair_rows(a.min.grad.score.pairs, b);
  const PairRows own = {rows.lo, rows.n, rows.lo, rows.n};
  const int n = rows.n;
  const float* x0 = a.min.x0 + 3 * (size_t)rows.lo;
  float* x = a.min.x_out + 3 * (size_t)rows.lo;
  const float* g_inter = a.min.grad.atom_grad + 3 * (size_t)rows.lo;
  const float* g_intra = a.intra.out.atom_grad + 3 * (size_t)rows.lo;
  VinaScoreArgs in = a.min.grad.score;                              // the scan for coordinates that are not finite reads the input
  in.pairs.lig_x = a.min.x0;
  if (vina_nonfinite(in, rows, b)) {
    const float nan = __builtin_nanf("");
    for (int k = tid; k < 3 * n; k += kThreads) {
      x[k] = x0[k];
      a.min.grad.atom_grad[3 * (size_t)rows.lo + k] = nan;
      a.intra.out.atom_grad[3 * (size_t)rows.lo + k] = nan;
    }
    for (int k = tid; k < kVinaTerms * n; k += kThreads) a.intra.out.score.atom_out[kVinaTerms * (size_t)rows.lo + k] = nan;
    if (tid < kVinaMolOut) a.intra.out.score.mol_out[(size_t)kVinaMolOut * b + tid] = nan;
    if (tid < kVinaMolGrad) a.min.grad.mol_grad[(size_t)kVinaMolGrad * b + tid] = nan;
    if (tid < kVinaMolPose) a.min.mol_pose[(size_t)kVinaMolPose * b + tid] = nan;
    if (tid < kVinaMolFlex) a.min.mol_min[(size_t)kVinaMolFlex * b + tid] = nan;
    if (tid < kVinaMolStat) a.min.mol_stat[(size_t)kVinaMolStat * b + tid] = tid == 0 ? (int)kVinaMinNonfinite : 0;
    if (tid < kVinaMaxTorsions) a.theta[(size_t)kVinaMaxTorsions * b + tid] = a.tau[(size_t)kVinaMaxTorsions * b + tid] = nan;
    if (tid == 0) a.intra.out.score.mol_flag[b] = 1;
    return;
  }
  if (tid == 0) {
    for (int k = 0; k < 3; ++k) st.t[k] = st.tt[k] = st.F[k] = st.M[k] = st.c[k] = 0.0;
    for (int k = 0; k < 4; ++k) st.q[k] = st.qt[k] = k == 0 ? 1.0 : 0.0;
    for (int k = 0; k < kVinaMaxTorsions; ++k) {
      st.th[k] = st.tht[k] = st.tau[k] = st.reach[k] = 0.0;
      st.rho2k[k] = 1.0;
    }
    st.rho2 = 1.0;
    st.rho_max = st.u = st.L = st.last_L = st.E = st.E_start = 0.0;
    st.inter_start = st.intra_start = 0.0f;
    st.evals = st.accepted = st.rejected = st.moved = 0;
    st.status = kVinaMinBudget;
    st.phase = kVinaMinFirst;
    // the rotors, range-checked; a molecule longer than the masks has none
    int kept = 0, K = 0;
    if ((a.dofs & kVinaDofTorsions) && n <= kMolMaxAtoms)
      kept = min(max(a.tor_int[(size_t)kVinaTorInt * b], 0), kVinaMaxTorsions);
    const VinaMask all = vina_mask_first(n);
    for (int k = 0; k < kept; ++k) {
      const int p = a.tor_end[((size_t)kVinaMaxTorsions * b + k) * 2], m = a.tor_end[((size_t)kVinaMaxTorsions * b + k) * 2 + 1];
      if (p < 0 || p >= n || m < 0 || m >= n || p == m) continue;
      VinaMask s = vina_mask_load(a.tor_side + ((size_t)kVinaMaxTorsions * b + k) * kVinaMaskWords);
      s.w[0] &= all.w[0];
      s.w[1] &= all.w[1];
      st.p[K] = p; st.m[K] = m; st.slot[K] = k; st.side[K] = s;
      ++K;
    }
    st.K = K;
    st.go = 1;
  }
  VinaGradPolicy pol{a.min.grad, {a.min.grad.score, nullptr}, part};
  VinaIntraPolicy intra_pol{a.intra, {a.intra.out, {a.intra.out.score, nullptr}, nullptr}, intra_part};
  for (int sweep = 0; sweep <= a.min.max_evals; ++sweep) {          // at most max_evals + 1 sweeps, whatever thread 0 decides
    __syncthreads();                                                // thread 0's pose and `go`; the sweeps before are over
    if (!__builtin_amdgcn_readfirstlane(st.go)) break;              // one LDS word, the same in every thread
    const int K = __builtin_amdgcn_readfirstlane(st.K);
    // the coordinates of the pose under evaluation
    double f[12];
    {
      double q[4];
      const double zero[3] = {0.0, 0.0, 0.0};
      for (int k = 0; k < 4; ++k) q[k] = st.qt[k];
      vina_min_frame(f, zero, zero, q);
      for (int k = 0; k < 3; ++k) f[9 + k] = st.tt[k];
    }
    if (K > 0) {                                                    // n <= kMolMaxAtoms
      if (tid < n)
        for (int k = 0; k < 3; ++k) y[tid][k] = (double)x0[3 * (size_t)tid + k];
      for (int r = 0; r < K; ++r) {
        __syncthreads();                                            // y as the rotors before left it
        const double angle = st.tht[r];
        const int p = st.p[r], m = st.m[r];
        double o[3], ax[3];
        for (int k = 0; k < 3; ++k) {
          o[k] = y[m][k];
          ax[k] = o[k] - y[p][k];
        }
        const double len = sqrt((ax[0] * ax[0] + ax[1] * ax[1]) + ax[2] * ax[2]);
        if (angle == 0.0 || !(len > 0.0)) continue;                 // the same in every thread
        const bool turns = tid < n && st.side[r].has(tid);
        double w[3] = {0, 0, 0};
        if (turns) {
          const double cs = cos(angle), sn = sin(angle);
          double v[3];
          for (int k = 0; k < 3; ++k) {
            ax[k] /= len;
            v[k] = y[tid][k] - o[k];
          }
          const double along = ((ax[0] * v[0] + ax[1] * v[1]) + ax[2] * v[2]) * (1.0 - cs);
          for (int k = 0; k < 3; ++k) {
            const double cr = ax[(k + 1) % 3] * v[(k + 2) % 3] - ax[(k + 2) % 3] * v[(k + 1) % 3];
            w[k] = o[k] + ((v[k] * cs + cr * sn) + ax[k] * along);
          }
        }
        __syncthreads();                                            // every thread has read the axis
        if (turns)
          for (int k = 0; k < 3; ++k) y[tid][k] = w[k];
      }
      __syncthreads();
      if (tid < n)
        for (int k = 0; k < 3; ++k)
          x[3 * (size_t)tid + k] = (float)(f[9 + k] + ((f[3 * k] * y[tid][0] + f[3 * k + 1] * y[tid][1]) + f[3 * k + 2] * y[tid][2]));
    } else {
      for (int i = tid; i < n; i += kThreads) {
        double s[3];
        for (int k = 0; k < 3; ++k) s[k] = (double)x0[3 * (size_t)i + k];
        for (int k = 0; k < 3; ++k)
          x[3 * (size_t)i + k] = (float)(f[9 + k] + ((f[3 * k] * s[0] + f[3 * k + 1] * s[1]) + f[3 * k + 2] * s[2]));
      }
    }
    __syncthreads();                                                // the coordinates, before any wave's sweep reads them
    pair_sweep(a.min.grad.score.pairs, rows, pol);
    pair_sweep(a.intra.out.score.pairs, own, intra_pol);
    if (tid == 0) vina_flex_judge(a, b, st);                        // reads the rows it stored itself in the two `finish`
    __syncthreads();                                                // `moved`, and every wave's gradient rows
    if (__builtin_amdgcn_readfirstlane(st.moved)) {                 // the geometry of the newly accepted pose, which x_out holds
      double c[3] = {0, 0, 0}, none = 0.0;
      for (int i = tid; i < n; i += kThreads)
        for (int k = 0; k < 3; ++k) c[k] += (double)x[3 * (size_t)i + k];
      vina_min_reduce(c, none, red);
      if (n > 0)
        for (int k = 0; k < 3; ++k) c[k] /= (double)n;
      double sq[3] = {0, 0, 0}, top = 0.0;
      for (int i = tid; i < n; i += kThreads) {
        double s2 = 0.0;
        for (int k = 0; k < 3; ++k) {
          const double s = (double)x[3 * (size_t)i + k] - c[k];
          s2 += s * s;
        }
        sq[0] += s2;
        top = fmax(top, s2);
      }
      vina_min_reduce(sq, top, red);
      if (tid == 0) {
        for (int k = 0; k < 3; ++k) st.c[k] = c[k];
        st.rho2 = n > 0 ? fmax(sq[0] / (double)n, 1.0) : 1.0;
        st.rho_max = sqrt(top);
      }
      for (int r = wave; r < K; r += kThreads / 64) {               // a wave per rotor, lanes over the atoms lane and lane + 64
        const int p = st.p[r], m = st.m[r];
        const VinaMask side = st.side[r];
        double o[3], ax[3];
        for (int k = 0; k < 3; ++k) {
          o[k] = (double)x[3 * (size_t)m + k];
          ax[k] = o[k] - (double)x[3 * (size_t)p + k];
        }
        const double len = sqrt((ax[0] * ax[0] + ax[1] * ax[1]) + ax[2] * ax[2]);
        double torque = 0.0, sum2 = 0.0, top2 = 0.0;
        if (len > 0.0) {
          for (int k = 0; k < 3; ++k) ax[k] /= len;
          for (int h = 0; h < 2; ++h) {
            const int i = lane + 64 * h;
            if (i >= n || !side.has(i)) continue;
            double v[3], g[3];
            for (int k = 0; k < 3; ++k) {
              v[k] = (double)x[3 * (size_t)i + k] - o[k];
              g[k] = (double)g_inter[3 * (size_t)i + k] + (double)g_intra[3 * (size_t)i + k];
            }
            double d2 = 0.0;
            for (int k = 0; k < 3; ++k) {
              const int k1 = (k + 1) % 3, k2 = (k + 2) % 3;
              torque += ax[k] * (v[k1] * g[k2] - v[k2] * g[k1]);
              const double e = v[k1] * ax[k2] - v[k2] * ax[k1];
              d2 += e * e;
            }
            sum2 += d2;
            top2 = fmax(top2, d2);
          }
        }
        for (int o2 = 32; o2; o2 >>= 1) {
          torque += __shfl_xor(torque, o2);
          sum2 += __shfl_xor(sum2, o2);
          top2 = fmax(top2, __shfl_xor(top2, o2));
        }
        if (lane == 0) {
          const int count = side.count();
          st.tau[r] = torque;
          st.reach[r] = sqrt(top2);
          st.rho2k[r] = count > 0 ? fmax(sum2 / (double)count, 1.0) : 1.0;
        }
      }
      __syncthreads();                                              // the scales and torques, before thread 0 reads them
    }
    if (tid == 0) vina_flex_step(a, b, st);
  }
  if (tid == 0) {
    float* pose = a.min.mol_pose + (size_t)kVinaMolPose * b;
    for (int k = 0; k < 3; ++k) pose[k] = (float)st.t[k];
    for (int k = 0; k < 4; ++k) pose[3 + k] = (float)st.q[k];
    pose[7] = (float)st.rho2;
    float* mn = a.min.mol_min + (size_t)kVinaMolFlex * b;
    mn[0] = st.inter_start;
    mn[1] = a.min.grad.score.mol_out[(size_t)kVinaMolOut * b + 5];
    mn[2] = (float)st.last_L;
    mn[3] = (float)st.u;
    mn[4] = st.intra_start;
    mn[5] = a.intra.out.score.mol_out[(size_t)kVinaMolOut * b + 5];
    mn[6] = (float)st.E_start;
    mn[7] = (float)st.E;
    int* stat = a.min.mol_stat + (size_t)kVinaMolStat * b;
    stat[0] = st.status; stat[1] = st.evals; stat[2] = st.accepted; stat[3] = 0;
    float* theta = a.theta + (size_t)kVinaMaxTorsions * b;
    float* tau = a.tau + (size_t)kVinaMaxTorsions * b;
    for (int k = 0; k < kVinaMaxTorsions; ++k) theta[k] = tau[k] = 0.0f;
    for (int k = 0; k < st.K; ++k) {
      theta[st.slot[k]] = (float)st.th[k];
      tau[st.slot[k]] = (float)st.tau[k];
    }
  }
}

}  // namespace dsbdd
