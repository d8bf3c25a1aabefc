// Launch helpers (host side, included by engine.hip): node GEMMs, the persistent grid and the H dispatch of the edge
// kernels, the radius-graph builder.
#pragma once

static hipError_t nl(hipStream_t s, const float* A1, int lda1, int K1, const float* A2, int lda2, int K2,
                     const float* WT, int ldw, const float* bias, const float* R, int ldr, float* C,
                     int ldc, int64_t M, int N, int act) {
  NodeLinearArgs a{A1, lda1, K1, A2, lda2, K2, WT, ldw, bias, R, ldr, C, ldc, (int)M, N, act, nullptr, nullptr};
  return launch_node_linear(s, a);
}

// one thread per item in workgroups of 256: the elementwise kernels.  The arguments are converted to the kernel's own
// parameter types (float* -> const float*, nullptr -> T*).
template <class... P, class... A>
static int launch_1d(void (*kernel)(P...), size_t n_items, hipStream_t s, A... args) {
  hipLaunchKernelGGL(kernel, dim3((unsigned)((n_items + 255) / 256)), dim3(256), 0, s, static_cast<P>(args)...);
  HIP_TRY(hipGetLastError());
  return DSBDD_OK;
}

static int device_cus() {      // CU count of the CURRENT device (cached per device id)
  static int cache[64] = {0};
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return 256;
  if (cache[dev] == 0) {
    hipDeviceProp_t pr;
    int n = 0;
    if (hipGetDeviceProperties(&pr, dev) == hipSuccess) n = pr.multiProcessorCount;
    cache[dev] = n > 0 ? n : 256;
  }
  return cache[dev];
}

// Grid of a persistent kernel: one workgroup per work item up to per_cu x n_cu resident ones (max_wg > 0: a lower cap,
// the DSBDD_EDGE_MAX_WG test hook), rounded up to a multiple of `quantum` (8 XCDs x MLPs), at least one quantum.
static int persistent_grid(int64_t items, int n_cu, int per_cu, int max_wg, int quantum) {
  int64_t resident = (int64_t)per_cu * n_cu;
  if (max_wg > 0 && max_wg < resident) resident = max_wg;
  if (items > resident) items = resident;
  const int grid = (int)((items + quantum - 1) / quantum * quantum);
  return grid < quantum ? quantum : grid;
}

template <int H>
static hipError_t launch_wave_emu_t(hipStream_t s, int mode, const EdgeArgs& a, int grid, int emu) {
  if (emu == 9) {
    if (mode == MODE_GCL) hipLaunchKernelGGL((edge_wave_kernel<H, MODE_GCL, false, 9>), dim3(grid), dim3(kThreads), 0, s, a);
    else hipLaunchKernelGGL((edge_wave_kernel<H, MODE_COORD, false, 9>), dim3(grid), dim3(kThreads), 0, s, a);
  } else {
    if (mode == MODE_GCL) hipLaunchKernelGGL((edge_wave_kernel<H, MODE_GCL, false, 6>), dim3(grid), dim3(kThreads), 0, s, a);
    else hipLaunchKernelGGL((edge_wave_kernel<H, MODE_COORD, false, 6>), dim3(grid), dim3(kThreads), 0, s, a);
  }
  return hipGetLastError();
}

template <int H>
static hipError_t launch_wave_t(hipStream_t s, int mode, const EdgeArgs& a, int grid) {
  // lane-grouped W2^T copies present (EdgeMlpW::W2TP): 16-byte B-operand reads
  constexpr bool can_perm = (H == 256 || H == 128);
  if constexpr (can_perm) {
    if (a.mlp[0].W2TP && a.mlp[1].W2TP) {
      if (mode == MODE_GCL)
        hipLaunchKernelGGL((edge_wave_kernel<H, MODE_GCL, true>), dim3(grid), dim3(kThreads), 0, s, a);
      else
        hipLaunchKernelGGL((edge_wave_kernel<H, MODE_COORD, true>), dim3(grid), dim3(kThreads), 0, s, a);
      return hipGetLastError();
    }
  }
  if (mode == MODE_GCL)
    hipLaunchKernelGGL((edge_wave_kernel<H, MODE_GCL, false>), dim3(grid), dim3(kThreads), 0, s, a);
  else
    hipLaunchKernelGGL((edge_wave_kernel<H, MODE_COORD, false>), dim3(grid), dim3(kThreads), 0, s, a);
  return hipGetLastError();
}

// training forward of the network path: the stage keeps z2 (edge_wave_kernel<.., STORE>)
template <int H>
static hipError_t launch_wave_store_t(hipStream_t s, int mode, const EdgeArgs& a, int grid) {
  if (mode == MODE_GCL) hipLaunchKernelGGL((edge_wave_kernel<H, MODE_GCL, false, 0, true>), dim3(grid), dim3(kThreads), 0, s, a);
  else hipLaunchKernelGGL((edge_wave_kernel<H, MODE_COORD, false, 0, true>), dim3(grid), dim3(kThreads), 0, s, a);
  return hipGetLastError();
}

template <int H>
static hipError_t launch_wave16_t(hipStream_t s, int mode, const EdgeArgs& a, int grid) {
  if (mode == MODE_GCL) hipLaunchKernelGGL((edge_wave16_kernel<H, MODE_GCL>), dim3(grid), dim3(kThreads), 0, s, a);
  else hipLaunchKernelGGL((edge_wave16_kernel<H, MODE_COORD>), dim3(grid), dim3(kThreads), 0, s, a);
  return hipGetLastError();
}

// 16-edge-granule variant (edge_wave16.h): 64-edge workgroup items, one per (tile, MLP), persistent over 2 workgroups per CU
static hipError_t launch_edge16(const dsbdd_engine* e, hipStream_t s, int mode, const EdgeArgs& a, int64_t edge_bound) {
  const int64_t items = (edge_bound + 63) / 64 * (mode == MODE_COORD ? a.n_mlp : 1);
  const int grid = persistent_grid(items, e->n_cu, 2, e->edge_max_wg, 1);
  return with_hidden(e->cfg.hidden_nf, [&](auto h) { return launch_wave16_t<decltype(h)::value>(s, mode, a, grid); });
}

// split-K variant (edge_splitk.h): one workgroup item per (32-edge tile, MLP), persistent over 2 workgroups per CU
static hipError_t launch_edge_sk(const dsbdd_engine* e, hipStream_t s, int mode, const EdgeArgs& a, int64_t edge_bound) {
  const bool two = mode == MODE_COORD && a.n_mlp == 2;
  const int64_t items = (edge_bound + 31) / 32 * (two ? 2 : 1);
  const int grid = persistent_grid(items, e->n_cu, 2, e->edge_max_wg, two ? 16 : 8);   // 8 XCDs (x 2 MLPs)
  if (e->cfg.hidden_nf != 256) return hipErrorInvalidValue;
  if (mode == MODE_GCL) hipLaunchKernelGGL((edge_splitk_kernel<256, MODE_GCL>), dim3(grid), dim3(kThreads), 0, s, a);
  else hipLaunchKernelGGL((edge_splitk_kernel<256, MODE_COORD>), dim3(grid), dim3(kThreads), 0, s, a);
  return hipGetLastError();
}

// 128-edge workgroup tiles (4 waves x 32 edges), 2 workgroups per CU, persistent over tiles
static int edge_wave_grid(int mode, const EdgeArgs& a, int64_t edge_bound, int n_cu, int max_wg) {
  const int64_t tiles = (edge_bound + 127) / 128;
  const bool split = mode == MODE_COORD && a.pass_split && a.n_mlp == 2;   // one workgroup per (tile, MLP)
  return persistent_grid(split ? 2 * tiles : tiles, n_cu, 2, max_wg, split ? 16 : 8);   // 8 XCDs (x 2 MLPs)
}

static hipError_t launch_edge(const dsbdd_engine* e, hipStream_t s, int mode, const EdgeArgs& a0,
                              int64_t edge_bound, bool g16 = false, bool sk = false) {
  if (sk && a0.mlp[0].W2SK) return launch_edge_sk(e, s, mode, a0, edge_bound);
  if (g16) return launch_edge16(e, s, mode, a0, edge_bound);
  int grid = edge_wave_grid(mode, a0, edge_bound, e->n_cu, e->edge_max_wg);
  const int emu = (e->emu && a0.mlp[0].W2E && a0.mlp[1].W2E) ? e->emu : 0;   // fp32 emulated on the bf16 matrix cores (engine option, opt-in)
  EdgeArgs a = a0;
  // quarter items (DSBDD_OPT_TAIL; edge_wave.h): the exact message kernels at hidden_nf 256 on the lane-grouped W2^T copy.
  // The rule's S is the resident grid (or the option's value, a test hook); a tile may take four workgroups.
  if (e->tail > 0 && mode == MODE_GCL && e->cfg.hidden_nf == 256 && !emu && a.mlp[0].W2TP && a.mlp[1].W2TP) {
    const int resident = persistent_grid(INT64_MAX / 2, e->n_cu, 2, e->edge_max_wg, 8);
    a.tail_s = e->tail > 1 ? e->tail : resident;
    grid = persistent_grid((edge_bound + 127) / 128 * 4, e->n_cu, 2, e->edge_max_wg, 8);
  }
  if (a.msg_out) {      // shell stage of the forward cone (forward.h): the default exact message kernel + the message store
    if (mode != MODE_GCL || e->cfg.hidden_nf != 256 || e->emu || !a.mlp[0].W2TP || a.wt_base) return hipErrorInvalidValue;
    hipLaunchKernelGGL((edge_wave_kernel<256, MODE_GCL, true, 0, false, true>), dim3(grid), dim3(kThreads), 0, s, a);
    return hipGetLastError();
  }
  return with_hidden(e->cfg.hidden_nf, [&](auto h) {
    constexpr int H = decltype(h)::value;
    return emu ? launch_wave_emu_t<H>(s, mode, a, grid, emu) : launch_wave_t<H>(s, mode, a, grid);
  });
}

// the edge stages of the training step (train_blocks.h): no engine, the current device's CU count, no grid cap
static hipError_t launch_edge_plain(int H, hipStream_t s, int mode, const EdgeArgs& a, int64_t edge_bound) {
  const int grid = edge_wave_grid(mode, a, edge_bound, device_cus(), 0);
  if (a.z2_out && (a.e_count_b || a.wt_base)) return hipErrorInvalidValue;
  return with_hidden(H, [&](auto h) {
    constexpr int HH = decltype(h)::value;
    return a.z2_out ? launch_wave_store_t<HH>(s, mode, a, grid) : launch_wave_t<HH>(s, mode, a, grid);
  });
}

static Cutoffs cutoffs_of(const dsbdd_config& c) {
  return Cutoffs{c.has_cutoff_ligand, c.has_cutoff_pocket, c.has_cutoff_interaction,
                 c.cutoff_ligand, c.cutoff_pocket, c.cutoff_interaction};
}

static int build_edges_impl(hipStream_t s, const float* x, int n_lig, int N, int B, const dsbdd_config& c,
                            const int* node_batch, const int* lig_off, const int* poc_off, int* deg,
                            int* row_ptr, int* erow, int* ecol, float* ed0, int64_t cap, int* status,
                            int* act_flag = nullptr, int* scan_tmp = nullptr, int* seg_base = nullptr,
                            const EdgeList2* list2 = nullptr, int id_offset = 0, int* lvl = nullptr) {
  const int waves_per_block = kThreads / 64;
  int blocks = (N + waves_per_block - 1) / waves_per_block;
  if (blocks > 4096) blocks = 4096;
  if (blocks < 1) blocks = 1;
  const Cutoffs cut = cutoffs_of(c);
  // with scan_tmp / seg_base: every (sample, node set) segment of the edge list starts at a wave-tile
  // boundary (radius_graph.h scan_kernel); without: a compact list (the public dsbdd_build_edges)
  const int aligned = scan_tmp && seg_base;
  SegAlign sg{node_batch, lig_off, poc_off, n_lig, B, scan_tmp, aligned ? seg_base : nullptr};
  EdgeList2 l2{};
  if (list2 && aligned) l2 = *list2;
  hipLaunchKernelGGL((edges_kernel<false>), dim3(blocks), dim3(kThreads), 0, s, x, node_batch, lig_off,
                     poc_off, n_lig, N, cut, deg, (const int*)nullptr, (int*)nullptr, (int*)nullptr,
                     (float*)nullptr, 0, status, act_flag, SegAlign{}, (int*)nullptr, l2, 0, lvl);
  HIP_TRY(hipGetLastError());
  hipLaunchKernelGGL(scan_kernel, dim3(l2.deg ? 2 : 1), dim3(1024), 0, s, (const int*)deg, row_ptr, N, sg,
                     (const int*)l2.deg, l2.row_ptr, l2.seg);
  HIP_TRY(hipGetLastError());
  hipLaunchKernelGGL((edges_kernel<true>), dim3(blocks), dim3(kThreads), 0, s, x, node_batch, lig_off,
                     poc_off, n_lig, N, cut, deg, (const int*)row_ptr, erow, ecol, ed0, (int)cap, status,
                     (int*)nullptr, sg, row_ptr, l2, id_offset, (int*)nullptr);
  HIP_TRY(hipGetLastError());
  return DSBDD_OK;
}
