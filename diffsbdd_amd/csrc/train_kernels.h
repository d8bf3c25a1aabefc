// Device side of the network training step (train_net.h): the batched weight re-layout and gradient-assembly kernels with
// their descriptor tables, and the elementwise kernels between the GEMMs.  Included by engine.hip next to train.h.
#pragma once

namespace dsbdd {

struct TnPackDesc {       // dT[c][r] = src[r][c] (ldT floats per row, padding columns zeroed), dP[r][c] = src[r][c]
  const float* src; int ld_src; int rows; int cols;
  float* dT; int ldT; int padT;     // padT: columns rows .. padT-1 of every dT row are cleared
  float* dP; int ldP;
};
struct TnTabDesc {        // tab[ty][o] = b1[o] + sum_e emb[ty][e] W1[o][col0 + e]
  const float* W1; int ld; int col0; const float* b1; const float* emb; int enf; float* tab; int H;
};
struct TnUnpackDesc {     // one edge MLP's first layer: d W1 [H][ld], d b1 [H], d emb partial [3][enf]
  float* dW1; int ld; float* db1; float* demb_part;      // (demb_part is scratch: always overwritten)
  const float* dWpq; int dq_off;      // d W_pq rows [0, H) = P part, rows [dq_off, dq_off + H) = Q part; [.][H]
  const float* d_vec;                 // [8][H]: d_wd, d_wd0, d_tab[0..2], ...
  const float* W1; const float* emb; int enf; int H;
  int acc_w, acc_b;                   // d W1 / d b1 += instead of =
};
struct TnCopyDesc { float* dst; const float* a; const float* b; int n; int acc; };    // dst[i] (+)= a[i] (+ b[i])
// The accumulating stores (dsbdd_train_net_backward_acc): the complete new gradient `v` first, the old value added last
// with ONE rounding; __fadd_rn keeps the compiler from contracting the add into the multiply that produced `v`.
__device__ __forceinline__ void tn_store(float* dst, float v, int acc) { *dst = acc ? __fadd_rn(*dst, v) : v; }
// The gradient-assembly tables travel BY VALUE in the kernel arguments (<= 4 KB): they depend on the per-call workspace,
// and a per-step host-to-device copy of a table would need either pinned memory or a synchronisation to be safe.
constexpr int kTnUnpackPerLaunch = 16, kTnCopyPerLaunch = 64;
struct TnUnpackTable { TnUnpackDesc d[kTnUnpackPerLaunch]; };
struct TnCopyTable { TnCopyDesc d[kTnCopyPerLaunch]; };

__global__ void tn_pack_kernel(const TnPackDesc* descs) {
  const TnPackDesc d = descs[blockIdx.y];
  const int total = d.rows * d.cols;
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < total; i += gridDim.x * blockDim.x) {
    const int r = i / d.cols, c = i % d.cols;
    const float v = d.src[(size_t)r * d.ld_src + c];
    if (d.dT) d.dT[(size_t)c * d.ldT + r] = v;
    if (d.dP) d.dP[(size_t)r * d.ldP + c] = v;
  }
  if (d.dT && d.padT > d.rows) {
    const int pw = d.padT - d.rows, tot = pw * d.cols;
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < tot; i += gridDim.x * blockDim.x)
      d.dT[(size_t)(i / pw) * d.ldT + d.rows + i % pw] = 0.f;
  }
  if (d.dP && d.ldP > d.cols) {
    const int pw = d.ldP - d.cols, tot = pw * d.rows;
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < tot; i += gridDim.x * blockDim.x)
      d.dP[(size_t)(i / pw) * d.ldP + d.cols + i % pw] = 0.f;
  }
}

__global__ void tn_tab_kernel(const TnTabDesc* descs) {
  const TnTabDesc d = descs[blockIdx.x];
  for (int i = threadIdx.x; i < 3 * d.H; i += blockDim.x) {
    const int ty = i / d.H, o = i % d.H;
    float v = d.b1[o];
    for (int e = 0; e < d.enf; ++e) v = fmaf(d.emb[ty * d.enf + e], d.W1[(size_t)o * d.ld + d.col0 + e], v);
    d.tab[i] = v;
  }
}

__global__ void tn_unpack_kernel(const TnUnpackTable tab) {
  const TnUnpackDesc& d = tab.d[blockIdx.y];
  const int H = d.H, ld = d.ld, total = H * ld;
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < total; i += gridDim.x * blockDim.x) {
    const int o = i / ld, c = i % ld;
    float v;
    if (c < H) v = d.dWpq[(size_t)o * H + c];
    else if (c < 2 * H) v = d.dWpq[(size_t)(d.dq_off + o) * H + (c - H)];
    else if (c == 2 * H) v = d.d_vec[o];
    else if (c == 2 * H + 1) v = d.d_vec[H + o];
    else {   // d W1[o][2H + 2 + e] = sum_ty d_tab[ty][o] emb[ty][e]
      const int e = c - 2 * H - 2;
      v = 0.f;
      for (int ty = 0; ty < 3; ++ty) v = fmaf(d.d_vec[(2 + ty) * H + o], d.emb[ty * d.enf + e], v);
    }
    tn_store(d.dW1 + i, v, d.acc_w);
  }
  if (blockIdx.x == 0) {
    for (int o = threadIdx.x; o < H; o += blockDim.x)
      tn_store(d.db1 + o, (d.d_vec[2 * H + o] + d.d_vec[3 * H + o]) + d.d_vec[4 * H + o], d.acc_b);
    if (d.demb_part)      // d emb[ty][e] = sum_o d_tab[ty][o] W1[o][2H + 2 + e], one thread per entry, fixed order
      for (int i = threadIdx.x; i < 3 * d.enf; i += blockDim.x) {
        const int ty = i / d.enf, e = i % d.enf;
        float v = 0.f;
        for (int o = 0; o < H; ++o) v = fmaf(d.d_vec[(2 + ty) * H + o], d.W1[(size_t)o * ld + 2 * H + 2 + e], v);
        d.demb_part[i] = v;
      }
  }
}

__global__ void tn_copy_kernel(const TnCopyTable tab) {
  const TnCopyDesc& d = tab.d[blockIdx.y];
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < d.n; i += gridDim.x * blockDim.x)
    tn_store(d.dst + i, d.b ? d.a[i] + d.b[i] : d.a[i], d.acc);
}

// out[i] = sum over k < n_part of part[k * stride + i] in order (the edge-type embedding's gradient over the MLPs)
__global__ void tn_sum_parts_kernel(const float* part, int n_part, int stride, int n, float* out, int acc) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  float v = 0.f;
  for (int k = 0; k < n_part; ++k) v += part[(size_t)k * stride + i];
  tn_store(out + i, v, acc);
}

// dynamics.py:89-93,100: x = cat(ligand, pocket coordinates), the feature parts as contiguous matrices
__global__ void tn_split_inputs_kernel(const float* xh_l, int dl, const float* xh_p, int dp, int n_l, int n_p, float* x0,
                                       float* hf_l, float* hf_p) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n_l + n_p) return;
  const bool lig = i < n_l;
  const float* src = lig ? xh_l + (size_t)i * dl : xh_p + (size_t)(i - n_l) * dp;
  const int nf = (lig ? dl : dp) - 3;
  float* hf = lig ? hf_l + (size_t)i * nf : hf_p + (size_t)(i - n_l) * nf;
  x0[3 * i] = src[0]; x0[3 * i + 1] = src[1]; x0[3 * i + 2] = src[2];
  for (int k = 0; k < nf; ++k) hf[k] = src[3 + k];
}

// dynamics.py:104-111: h = cat[h, t[mask]]; the padding columns of the row are cleared
__global__ void tn_time_col_kernel(float* h0, int JP, int J, const float* t, int t_count, const int* node_batch, int N) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= N) return;
  h0[(size_t)i * JP + J] = t[t_count == 1 ? 0 : node_batch[i]];
  for (int k = J + 1; k < JP; ++k) h0[(size_t)i * JP + k] = 0.f;
}

__global__ void tn_silu_kernel(const float* z, float* a, size_t n) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) a[i] = silu(z[i]);
}
__global__ void tn_silu_bwd_kernel(const float* da, const float* z, float* dz, size_t n) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) { const float zz = z[i]; dz[i] = da[i] * dsilu_from(zz, sigmoidf_fast(zz)); }
}
__global__ void tn_add_kernel(float* dst, const float* src, size_t n) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) dst[i] += src[i];
}
__global__ void tn_sub_kernel(float* dst, const float* src, size_t n) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) dst[i] -= src[i];
}
__global__ void tn_cat_kernel(const float* h, const float* agg, float* out, int N, int H) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (size_t)N * 2 * H) return;
  const int r = (int)(i / (2 * H)), c = (int)(i % (2 * H));
  out[i] = c < H ? h[(size_t)r * H + c] : agg[(size_t)r * H + c - H];
}
// vel = x_final - x_in (dynamics.py:136); NaN -> 0 in training, status bit 1 otherwise (:155-159)
__global__ void tn_vel_kernel(const float* x_fin, const float* x0, float* vel, int n3, int zero_nan, int* status) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n3) return;
  float v = x_fin[i] - x0[i];
  if (v != v) { if (zero_nan) v = 0.f; else atomicOr(status, 1); }
  vel[i] = v;
}
// eps = cat[vel (- per-sample mean in joint mode, dynamics.py:161-164), decoded features]
__global__ void tn_out_kernel(const float* vel, const float* meanv, const int* node_batch, const float* eh_l, int a,
                              const float* eh_p, int r, int n_l, int n_p, float* eps_l, float* eps_p) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n_l + n_p) return;
  const bool lig = i < n_l;
  const int nf = lig ? a : r;
  float* dst = lig ? eps_l + (size_t)i * (3 + a) : eps_p + (size_t)(i - n_l) * (3 + r);
  const float* eh = lig ? eh_l + (size_t)i * a : eh_p + (size_t)(i - n_l) * r;
  const int b = node_batch[i];
  for (int k = 0; k < 3; ++k) dst[k] = vel[3 * i + k] - (meanv ? meanv[3 * b + k] : 0.f);
  for (int k = 0; k < nf; ++k) dst[3 + k] = eh[k];
}
// the reverse: d_vel (joint: minus its per-sample mean, applied by the caller through meanv) and the feature gradients
__global__ void tn_split_grads_kernel(const float* d_l, int a, const float* d_p, int r, int n_l, int n_p, float* d_vel,
                                      float* deh_l, float* deh_p) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n_l + n_p) return;
  const bool lig = i < n_l;
  const int nf = lig ? a : r;
  const float* src = lig ? d_l + (size_t)i * (3 + a) : d_p + (size_t)(i - n_l) * (3 + r);
  float* dh = lig ? deh_l + (size_t)i * a : deh_p + (size_t)(i - n_l) * r;
  for (int k = 0; k < 3; ++k) d_vel[3 * i + k] = src[k];
  for (int k = 0; k < nf; ++k) dh[k] = src[3 + k];
}
// x[i] -= m[batch(i)]   (the mean-removal of a vector field and its transpose are the same map)
__global__ void tn_sub_mean_kernel(float* x, const float* m, const int* node_batch, int N) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= 3 * N) return;
  x[i] -= m[3 * node_batch[i / 3] + i % 3];
}
// SampleMean backward: d_x[i] += d_mean[b] / (number of nodes of sample b)
__global__ void tn_mean_bwd_kernel(float* d_x, const float* d_mean, const int* node_batch, const int* lig_off,
                                   const int* poc_off, int N) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= 3 * N) return;
  const int b = node_batch[i / 3];
  const int cnt = (lig_off[b + 1] - lig_off[b]) + (poc_off[b + 1] - poc_off[b]);
  d_x[i] += d_mean[3 * b + i % 3] / (float)(cnt > 0 ? cnt : 1);
}
// d_hout's time column (dropped by dynamics.py:147-149) and padding carry no gradient
__global__ void tn_clear_cols_kernel(float* m, int ld, int c0, int N) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= N) return;
  for (int k = c0; k < ld; ++k) m[(size_t)i * ld + k] = 0.f;
}
// d_xh = cat[d_x, d_hf]
__global__ void tn_join_grads_kernel(const float* d_x, const float* dhf_l, int a, const float* dhf_p, int r, int n_l,
                                     int n_p, float* d_l, float* d_p) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n_l + n_p) return;
  const bool lig = i < n_l;
  const int nf = lig ? a : r;
  float* dst = lig ? (d_l ? d_l + (size_t)i * (3 + a) : nullptr) : (d_p ? d_p + (size_t)(i - n_l) * (3 + r) : nullptr);
  if (!dst) return;
  const float* dh = lig ? dhf_l + (size_t)i * a : dhf_p + (size_t)(i - n_l) * r;
  for (int k = 0; k < 3; ++k) dst[k] = d_x[3 * i + k];
  for (int k = 0; k < nf; ++k) dst[3 + k] = dh[k];
}

}  // namespace dsbdd
