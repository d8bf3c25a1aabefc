// C-ABI wrappers of the native training loop around the network call (included by engine.hip): the loss terms of the
// pocket-conditioned step (loss_head.h), the fused clipping + AdamW step (optim.h), the auxiliary LJ loss (lj_loss.h).
#pragma once

static LossCfg loss_cfg_of(const dsbdd_loss_cfg* c) {
  return LossCfg{c->batch, c->n_lig, c->n_pocket, c->atom_nf, c->residue_nf, c->timesteps, c->remove_com, c->vnode_idx,
                 c->norm_value_x, c->norm_value_h, c->norm_bias_h, c->n1_tab, c->n2_tab};
}
static bool loss_cfg_ok(const dsbdd_loss_cfg* c) {
  return c && c->batch > 0 && c->n_lig >= 0 && c->n_pocket >= 0 && c->atom_nf > 0 && c->residue_nf > 0 && c->timesteps > 0 &&
         c->norm_value_x > 0.f && c->norm_value_h > 0.f && c->vnode_idx < c->atom_nf;
}

extern "C" {

int dsbdd_edge_capacity(void* stream, const int64_t* lig_mask, int64_t n_lig, const int64_t* pocket_mask, int64_t n_pocket,
                        int64_t batch, int64_t* out) {
  StreamDevice stream_device_(stream);
  if (!out || batch < 1 || n_lig < 0 || n_pocket < 0 || (n_lig > 0 && !lig_mask) || (n_pocket > 0 && !pocket_mask))
    return fail(DSBDD_ERR_ARG, "bad argument");
  hipLaunchKernelGGL(edge_capacity_kernel, dim3(1), dim3(kLossThreads), 0, static_cast<hipStream_t>(stream),
                     reinterpret_cast<const long long*>(lig_mask), (int)n_lig, reinterpret_cast<const long long*>(pocket_mask),
                     (int)n_pocket, (int)batch, reinterpret_cast<long long*>(out));
  HIP_TRY(hipGetLastError());
  return DSBDD_OK;
}

int dsbdd_loss_rows(void) { return LS_ROWS; }
int dsbdd_loss_out_rows(void) { return LO_ROWS; }

int dsbdd_loss_cond_pre(void* stream, const dsbdd_loss_cfg* cfg, const float* lig_x, const float* lig_h, const int64_t* lig_mask,
                        const float* pocket_x, const float* pocket_h, const int64_t* pocket_mask, const float* eps,
                        const float* t_int, const float* gamma_table, const float* logpn_table, float* z_t, float* xh_pocket,
                        float* per_sample, float* lig_x_norm, float* lig_h_norm, float* pocket_x_norm, float* pocket_h_norm) {
  StreamDevice stream_device_(stream);
  if (!loss_cfg_ok(cfg) || !t_int || !gamma_table || !per_sample || (cfg->n_lig > 0 && (!lig_x || !lig_h || !lig_mask || !eps || !z_t)) ||
      (cfg->n_pocket > 0 && (!pocket_x || !pocket_h || !pocket_mask || !xh_pocket)) || (logpn_table && (cfg->n1_tab < 1 || cfg->n2_tab < 1)))
    return fail(DSBDD_ERR_ARG, "bad argument");
  hipLaunchKernelGGL(loss_cond_pre_kernel, dim3((unsigned)cfg->batch), dim3(kLossThreads), 0, static_cast<hipStream_t>(stream),
                     loss_cfg_of(cfg), lig_x, lig_h, reinterpret_cast<const long long*>(lig_mask), pocket_x, pocket_h,
                     reinterpret_cast<const long long*>(pocket_mask), eps, t_int, gamma_table, logpn_table, z_t, xh_pocket, per_sample,
                     lig_x_norm, lig_h_norm, pocket_x_norm, pocket_h_norm);
  HIP_TRY(hipGetLastError());
  return DSBDD_OK;
}

int dsbdd_loss_cond_post(void* stream, const dsbdd_loss_cfg* cfg, const float* net, const float* eps, const float* z_t,
                         const float* lig_h, const int64_t* lig_mask, const float* per_sample, float* xh_hat, float* out) {
  StreamDevice stream_device_(stream);
  if (!loss_cfg_ok(cfg) || !per_sample || !out || (cfg->n_lig > 0 && (!net || !eps || !z_t || !lig_h || !lig_mask || !xh_hat)))
    return fail(DSBDD_ERR_ARG, "bad argument");
  hipLaunchKernelGGL(loss_cond_post_kernel, dim3((unsigned)cfg->batch), dim3(kLossThreads), 0, static_cast<hipStream_t>(stream),
                     loss_cfg_of(cfg), net, eps, z_t, lig_h, reinterpret_cast<const long long*>(lig_mask), per_sample, xh_hat, out);
  HIP_TRY(hipGetLastError());
  return DSBDD_OK;
}

int dsbdd_loss_cond_post_backward(void* stream, const dsbdd_loss_cfg* cfg, const float* net, const float* eps, const float* lig_h,
                                  const int64_t* lig_mask, const float* per_sample, const float* g_err, const float* g_l0x,
                                  const float* g_hat, float* d_net) {
  StreamDevice stream_device_(stream);
  if (!loss_cfg_ok(cfg) || !per_sample || (cfg->n_lig > 0 && (!net || !eps || !lig_h || !lig_mask || !d_net)))
    return fail(DSBDD_ERR_ARG, "bad argument");
  if (cfg->n_lig == 0) return DSBDD_OK;
  const size_t n = (size_t)cfg->n_lig * (3 + cfg->atom_nf);
  unsigned grid = (unsigned)((n + kLossThreads - 1) / kLossThreads);
  if (grid > 1024) grid = 1024;
  hipLaunchKernelGGL(loss_cond_post_bwd_kernel, dim3(grid), dim3(kLossThreads), 0, static_cast<hipStream_t>(stream),
                     loss_cfg_of(cfg), net, eps, lig_h, reinterpret_cast<const long long*>(lig_mask), per_sample, g_err, g_l0x,
                     g_hat, d_net);
  HIP_TRY(hipGetLastError());
  return DSBDD_OK;
}

}  // extern "C"

struct dsbdd_optim {
  dsbdd_optim_cfg cfg;
  std::vector<int64_t> numel, offset;     // per tensor; offsets into the flat m / v / vmax buffers (multiples of 4)
  std::vector<int> chunk_first;           // first chunk of every tensor, [n + 1]
  std::vector<OptimChunk> chunks;
  int64_t flat_elems = 0;
  float *m = nullptr, *v = nullptr, *vmax = nullptr;
  OptimChunk* d_chunks = nullptr;
  float** d_params = nullptr;
  double *d_partial = nullptr, *d_queue = nullptr, *d_scratch = nullptr;
  bool bound = false, has_params = false;
  int64_t n_steps = 0;                    // optimiser steps so far: its parity selects the queue that is read
  int n_cu = 256;
};

struct OptimWs { size_t chunks, params, partial, queue, scratch, total; };
static OptimWs optim_carve(const dsbdd_optim* o) {
  OptimWs w;
  size_t off = 0;
  w.chunks = off; off += al256(o->chunks.size() * sizeof(OptimChunk));
  w.params = off; off += al256(o->numel.size() * sizeof(float*));
  w.partial = off; off += al256(o->chunks.size() * sizeof(double));
  w.queue = off; off += al256(2 * kQueueStride * sizeof(double));
  w.scratch = off; off += 256;
  w.total = off;
  return w;
}

extern "C" {

int dsbdd_optim_create(const dsbdd_optim_cfg* cfg, int32_t n_tensors, const int64_t* numel, dsbdd_optim** out) {
  if (!cfg || !numel || !out || n_tensors < 1) return fail(DSBDD_ERR_ARG, "bad argument");
  if (!(cfg->lr >= 0.0) || !(cfg->beta1 >= 0.0 && cfg->beta1 < 1.0) || !(cfg->beta2 >= 0.0 && cfg->beta2 < 1.0) ||
      !(cfg->eps >= 0.0) || !(cfg->weight_decay >= 0.0))
    return fail(DSBDD_ERR_ARG, "bad hyper-parameter");
  if (1.0 - cfg->beta1 >= 0.5) return fail(DSBDD_ERR_ARG, "beta1 must be above 0.5 (lerp branch of the update kernel)");
  dsbdd_optim* o = new dsbdd_optim();
  o->cfg = *cfg;
  int64_t flat = 0;
  for (int i = 0; i < n_tensors; ++i) {
    if (numel[i] < 1) { delete o; return fail(DSBDD_ERR_ARG, "empty tensor " + std::to_string(i)); }
    o->numel.push_back(numel[i]);
    o->offset.push_back(flat);
    o->chunk_first.push_back((int)o->chunks.size());
    for (int64_t e = 0; e < numel[i]; e += kOptimChunk) {
      const int64_t cnt = numel[i] - e < kOptimChunk ? numel[i] - e : kOptimChunk;
      if (flat + e + cnt >= (1ll << 31)) { delete o; return fail(DSBDD_ERR_ARG, "more than 2^31 parameters"); }
      o->chunks.push_back(OptimChunk{i, (int)e, (int)cnt, (int)(flat + e)});
    }
    flat += (numel[i] + 3) & ~(int64_t)3;
  }
  o->chunk_first.push_back((int)o->chunks.size());
  o->flat_elems = flat;
  int dev = 0;
  hipDeviceProp_t prop;
  if (hipGetDevice(&dev) == hipSuccess && hipGetDeviceProperties(&prop, dev) == hipSuccess && prop.multiProcessorCount > 0)
    o->n_cu = prop.multiProcessorCount;
  else
    (void)hipGetLastError();
  *out = o;
  return DSBDD_OK;
}

void dsbdd_optim_destroy(dsbdd_optim* o) { delete o; }

int64_t dsbdd_optim_state_elems(const dsbdd_optim* o) { return o ? o->flat_elems : 0; }
int64_t dsbdd_optim_state_offset(const dsbdd_optim* o, int32_t tensor) {
  return (o && tensor >= 0 && tensor < (int)o->offset.size()) ? o->offset[tensor] : -1;
}
size_t dsbdd_optim_workspace_bytes(const dsbdd_optim* o) { return o ? optim_carve(o).total : 0; }

static void optim_queue_image(double* q, const double* items, int n, double clips, double steps) {
  for (int i = 0; i < kQueueStride; ++i) q[i] = 0.0;
  for (int i = 0; i < n; ++i) q[i] = items[n - 1 - i];         // items arrive newest first (utils.Queue.items); slot 0 = oldest
  q[QS_LEN] = (double)n;
  q[QS_HEAD] = (double)(n == kQueueLen ? 0 : n);
  q[QS_CLIPS] = clips;
  q[QS_STEPS] = steps;
}

int dsbdd_optim_bind(dsbdd_optim* o, void* stream, float* m, float* v, float* vmax, void* ws, size_t ws_bytes) {
  StreamDevice stream_device_(stream);
  if (!o || !m || !v || !vmax || !ws) return fail(DSBDD_ERR_ARG, "null argument");
  if ((reinterpret_cast<uintptr_t>(m) | reinterpret_cast<uintptr_t>(v) | reinterpret_cast<uintptr_t>(vmax)) & 15)
    return fail(DSBDD_ERR_ARG, "state buffers must be 16-byte aligned");
  if (reinterpret_cast<uintptr_t>(ws) & 255) return fail(DSBDD_ERR_ARG, "workspace must be 256-byte aligned");
  const OptimWs w = optim_carve(o);
  if (ws_bytes < w.total) return fail(DSBDD_ERR_CAPACITY, "workspace too small");
  hipStream_t s = static_cast<hipStream_t>(stream);
  char* b = static_cast<char*>(ws);
  o->m = m; o->v = v; o->vmax = vmax;
  o->d_chunks = reinterpret_cast<OptimChunk*>(b + w.chunks);
  o->d_params = reinterpret_cast<float**>(b + w.params);
  o->d_partial = reinterpret_cast<double*>(b + w.partial);
  o->d_queue = reinterpret_cast<double*>(b + w.queue);
  o->d_scratch = reinterpret_cast<double*>(b + w.scratch);
  double q[2 * kQueueStride];
  const double first = 3000.0;                                  // "Add large value that will be flushed."
  optim_queue_image(q, &first, 1, 0.0, 0.0);
  optim_queue_image(q + kQueueStride, &first, 1, 0.0, 0.0);
  HIP_TRY(hipMemcpyAsync(o->d_chunks, o->chunks.data(), o->chunks.size() * sizeof(OptimChunk), hipMemcpyHostToDevice, s));
  HIP_TRY(hipMemcpyAsync(o->d_queue, q, sizeof(q), hipMemcpyHostToDevice, s));
  HIP_TRY(hipMemsetAsync(o->d_partial, 0, o->chunks.size() * sizeof(double), s));
  HIP_TRY(hipMemsetAsync(o->d_scratch, 0, 256, s));
  HIP_TRY(hipStreamSynchronize(s));                             // the sources are host temporaries
  o->n_steps = 0;
  o->bound = true;
  o->has_params = false;
  return DSBDD_OK;
}

int dsbdd_optim_set_params(dsbdd_optim* o, void* stream, float* const* params) {
  StreamDevice stream_device_(stream);
  if (!o || !params) return fail(DSBDD_ERR_ARG, "null argument");
  if (!o->bound) return fail(DSBDD_ERR_STATE, "optimiser state not bound");
  for (size_t i = 0; i < o->numel.size(); ++i)
    if (!params[i] || (reinterpret_cast<uintptr_t>(params[i]) & 3))
      return fail(DSBDD_ERR_ARG, "parameter " + std::to_string(i) + " is null or misaligned");
  hipStream_t s = static_cast<hipStream_t>(stream);
  HIP_TRY(hipMemcpyAsync(o->d_params, params, o->numel.size() * sizeof(float*), hipMemcpyHostToDevice, s));
  HIP_TRY(hipStreamSynchronize(s));
  o->has_params = true;
  return DSBDD_OK;
}

int dsbdd_optim_step(dsbdd_optim* o, void* stream, const float* const* grads, const int32_t* steps, double lr) {
  StreamDevice stream_device_(stream);
  if (!o || !grads || !steps) return fail(DSBDD_ERR_ARG, "null argument");
  if (!o->bound || !o->has_params) return fail(DSBDD_ERR_STATE, "optimiser state or parameters not bound");
  if (!(lr >= 0.0)) return fail(DSBDD_ERR_ARG, "bad learning rate");
  hipStream_t s = static_cast<hipStream_t>(stream);
  const int n = (int)o->numel.size();
  const dsbdd_optim_cfg& c = o->cfg;
  OptimLaunch L{};
  L.chunks = o->d_chunks; L.n_chunks = (int)o->chunks.size(); L.params = o->d_params;
  L.m = o->m; L.v = o->v; L.vmax = o->vmax; L.partial = o->d_partial; L.queue = o->d_queue; L.scratch = o->d_scratch;
  L.parity = (int)(o->n_steps & 1); L.clip = c.clip_grad ? 1 : 0;
  // the scalars torch derives in Python doubles and hands to float32 kernels
  L.decay = (float)(1.0 - lr * c.weight_decay); L.w1 = (float)(1.0 - c.beta1); L.beta2 = (float)c.beta2;
  L.w2 = (float)(1.0 - c.beta2); L.eps = (float)c.eps;
  for (int pass = c.clip_grad ? 0 : 1; pass < 2; ++pass) {
    for (int lo = 0; lo < n; lo += kOptimTensors) {
      const int hi = lo + kOptimTensors < n ? lo + kOptimTensors : n;
      OptimStepArgs A{};
      for (int i = lo; i < hi; ++i) {
        A.grad[i - lo] = grads[i];
        if (!grads[i]) continue;
        if (steps[i] < 1) return fail(DSBDD_ERR_ARG, "step count of tensor " + std::to_string(i) + " must be >= 1");
        if (reinterpret_cast<uintptr_t>(grads[i]) & 3) return fail(DSBDD_ERR_ARG, "misaligned gradient");
        const double bc1 = 1.0 - std::pow(c.beta1, (double)steps[i]), bc2 = 1.0 - std::pow(c.beta2, (double)steps[i]);
        A.step_size_neg[i - lo] = (float)(-(lr / bc1));
        A.bc2_sqrt[i - lo] = (float)std::pow(bc2, 0.5);
      }
      L.tensor_lo = lo; L.chunk_lo = o->chunk_first[lo]; L.chunk_hi = o->chunk_first[hi]; L.first = lo == 0;
      int grid = L.chunk_hi - L.chunk_lo;
      if (grid > 2 * o->n_cu) grid = 2 * o->n_cu;
      if (grid < 1) grid = 1;
      if (pass == 0) hipLaunchKernelGGL(optim_norm_kernel, dim3(grid), dim3(kOptimThreads), 0, s, L, A);
      else hipLaunchKernelGGL(optim_update_kernel, dim3(grid), dim3(kOptimThreads), 0, s, L, A);
      HIP_TRY(hipGetLastError());
    }
  }
  if (c.clip_grad) ++o->n_steps;
  return DSBDD_OK;
}

int dsbdd_optim_state_read(dsbdd_optim* o, void* stream, double* out, int32_t capacity) {
  StreamDevice stream_device_(stream);
  if (!o || !out || capacity < kQueueStride) return fail(DSBDD_ERR_ARG, "bad argument");
  if (!o->bound) return fail(DSBDD_ERR_STATE, "optimiser state not bound");
  hipStream_t s = static_cast<hipStream_t>(stream);
  double q[kQueueStride];
  HIP_TRY(hipMemcpyAsync(q, o->d_queue + (o->n_steps & 1) * kQueueStride, sizeof(q), hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  // out: [0] number of entries, [1 .. 50] the entries newest first, then clips, last norm, last threshold, steps, last coefficient
  int len = (int)q[QS_LEN], head = (int)q[QS_HEAD];
  if (len < 0 || len > kQueueLen || head < 0 || head >= kQueueLen) return fail(DSBDD_ERR_STATE, "corrupt queue record");
  for (int i = 0; i < kQueueStride; ++i) out[i] = 0.0;
  out[0] = (double)len;
  for (int i = 0; i < len; ++i) out[1 + i] = q[(head - 1 - i + 2 * kQueueLen) % kQueueLen];
  out[51] = q[QS_CLIPS]; out[52] = q[QS_LAST_NORM]; out[53] = q[QS_LAST_MAX]; out[54] = q[QS_STEPS]; out[55] = q[QS_LAST_COEF];
  return DSBDD_OK;
}

int dsbdd_optim_state_write(dsbdd_optim* o, void* stream, const double* items, int32_t n_items, double clips, double steps) {
  StreamDevice stream_device_(stream);
  if (!o || !items || n_items < 1 || n_items > kQueueLen) return fail(DSBDD_ERR_ARG, "the queue holds 1 to 50 entries");
  if (!o->bound) return fail(DSBDD_ERR_STATE, "optimiser state not bound");
  hipStream_t s = static_cast<hipStream_t>(stream);
  double q[kQueueStride];
  optim_queue_image(q, items, n_items, clips, steps);
  HIP_TRY(hipMemcpyAsync(o->d_queue + (o->n_steps & 1) * kQueueStride, q, sizeof(q), hipMemcpyHostToDevice, s));
  HIP_TRY(hipStreamSynchronize(s));
  return DSBDD_OK;
}

int dsbdd_lj_potential(void* stream, const float* xh, int32_t ld, int32_t n_types, const int64_t* mask, int64_t n, int64_t batch,
                       const double* sigma, double clamp, int32_t has_clamp, int32_t* type_scratch, float* u, float* dx) {
  StreamDevice stream_device_(stream);
  if (batch < 1 || n < 0 || n >= (1ll << 30) || n_types < 1 || ld < 3 + n_types || !sigma || !u ||
      (n > 0 && (!xh || !mask || !type_scratch || !dx)))
    return fail(DSBDD_ERR_ARG, "bad argument");
  LjArgs a{xh, ld, n_types, reinterpret_cast<const long long*>(mask), (int)n, (int)batch, sigma, clamp, has_clamp, type_scratch, u, dx};
  hipLaunchKernelGGL(lj_potential_kernel, dim3((unsigned)batch), dim3(kLjThreads), 0, static_cast<hipStream_t>(stream), a);
  HIP_TRY(hipGetLastError());
  return DSBDD_OK;
}

}  // extern "C"
