// Virtual shards of a solver (solver_state.hpp; DESIGN.md 8 "one GPU") and what goes with them: the replicas'
// buffers, the CU budget, the merge period, the job's sample count, and the links between solvers whose replicas
// are averaged inside the fused epoch kernel -- peer access inside one process (sgdnet_solver_link_peers), hipIpc
// mappings between processes (sgdnet_solver_peer_info / _link_ipc).
#include <string.h>

#include <hip/hip_ext.h>

#include "solver_state.hpp"

using namespace sgdnet;

// the solver has no shards (and no links: they name the replicas' buffers)
static void free_virtual_shards(sgdnet_solver* s) {
  for (void* q : s->vs_owned) (void)hipFree(q);
  s->vs_owned.clear();
  SagaDev& d = s->d;
  d.V = 0;
  d.vw = d.vG = d.vb = d.vgb = d.vd0 = d.vref = d.vcw = d.vx = d.vpub = nullptr;
  d.vsync = d.vcol = nullptr;
  d.peers = nullptr;                            // links name the buffers just freed: link again
  d.n_peers = 0;
}

extern "C" {

int sgdnet_solver_set_virtual_shards(sgdnet_solver* s, int n_shards) {
  if (!s || n_shards < 0 || n_shards > 8) {
    set_error("sgdnet_solver_set_virtual_shards: 0..8 shards");
    return SGDNET_EINVAL;
  }
  SGD_HIP_TRY(hipSetDevice(s->device));
  SGD_HIP_TRY(hipStreamSynchronize(s->st));
  drop_graph(s);
  free_virtual_shards(s);
  SagaDev& d = s->d;
  if (n_shards < 2) return SGDNET_OK;
  if (d.K > 16) {
    set_error("virtual shards: up to 16 classes");
    return SGDNET_EUNSUPPORTED;
  }
  const int64_t KP = (int64_t)d.K * d.p;
  auto alloc = [&](double** out, size_t count) -> int {
    void* q = nullptr;
    if (hipMalloc(&q, sizeof(double) * count) != hipSuccess) return SGDNET_ENOMEM;
    (void)hipMemset(q, 0, sizeof(double) * count);
    s->vs_owned.push_back(q);
    *out = static_cast<double*>(q);
    return SGDNET_OK;
  };
  int rc = alloc(&d.vw, (size_t)n_shards * KP);
  if (!rc) rc = alloc(&d.vG, (size_t)n_shards * KP);
  if (!rc) rc = alloc(&d.vb, 8 * (size_t)d.K);
  if (!rc) rc = alloc(&d.vgb, 8 * (size_t)d.K);
  if (!rc) rc = alloc(&d.vcw, 8 * (size_t)d.K);
  if (!rc) rc = alloc(&d.vd0, 256 * (size_t)d.K);
  if (!rc) rc = alloc(&d.vref, (size_t)(2 * KP + 2 * d.K));
  if (!rc && d.K == 1) {
    // the fused epoch kernel's barrier counters and reference copies (ordinary device memory), and what its merges
    // exchange -- slice counters and published slices -- in fine-grained memory: linked solvers on other GPUs add to
    // those counters and read those slices while the kernels run (sgdnet_solver_link_peers)
    auto alloc_fg = [&](void** out, size_t bytes) -> int {
      void* q = nullptr;
      if (hipExtMallocWithFlags(&q, bytes, hipDeviceMallocFinegrained) != hipSuccess) {
        (void)hipGetLastError();
        if (hipMalloc(&q, bytes) != hipSuccess) return SGDNET_ENOMEM;   // (one GPU: any device memory will do)
      }
      (void)hipMemset(q, 0, bytes);
      s->vs_owned.push_back(q);
      *out = q;
      return SGDNET_OK;
    };
    double* words = nullptr;
    rc = alloc(&words, (vs_fused_sync_words() * sizeof(unsigned) + sizeof(double) - 1) / sizeof(double));
    d.vsync = reinterpret_cast<unsigned*>(words);
    if (!rc) rc = alloc(&d.vx, vs_fused_exchange_doubles(d, n_shards));
    if (!rc) rc = alloc_fg(reinterpret_cast<void**>(&d.vcol), vs_fused_col_words() * sizeof(unsigned));
    if (!rc) rc = alloc_fg(reinterpret_cast<void**>(&d.vpub), vs_fused_publish_doubles(d, n_shards) * sizeof(double));
  }
  if (rc) {
    set_error("virtual shards: out of device memory");
    return rc;
  }
  d.V = n_shards;
  d.v_bps = lds_target_grid(d) / n_shards;
  // shard v owns the samples [v * base + min(v, rem), ...): sgdnet_amd/parallel.py shard_bounds
  const int64_t base = d.n / n_shards, rem = d.n % n_shards;
  for (int v = 0; v < 8; ++v) d.v_size[v] = v < n_shards ? (double)(base + (v < rem ? 1 : 0)) : 0.0;
  if (!vs_eligible(d)) {   // the gather forms that carry shards keep their tables in LDS
    free_virtual_shards(s);
    set_error("virtual shards: n_features too large for the LDS-resident gather");
    return SGDNET_EUNSUPPORTED;
  }
  return SGDNET_OK;
}

int sgdnet_solver_set_cu_budget(sgdnet_solver* s, int cus) {
  if (!s || cus < 0) return SGDNET_EINVAL;
  SGD_HIP_TRY(hipSetDevice(s->device));
  SGD_HIP_TRY(hipStreamSynchronize(s->st));
  s->d.cu_budget = cus;
  if (s->d.V > 1) s->d.v_bps = lds_target_grid(s->d) / s->d.V;
  drop_graph(s);
  return SGDNET_OK;
}

int sgdnet_solver_set_merge_period(sgdnet_solver* s, int64_t draws_per_shard) {
  if (!s || draws_per_shard < 0) return SGDNET_EINVAL;
  SGD_HIP_TRY(hipSetDevice(s->device));
  SGD_HIP_TRY(hipStreamSynchronize(s->st));
  s->vs_period = draws_per_shard;
  drop_graph(s);
  return SGDNET_OK;
}

int sgdnet_solver_set_n_total(sgdnet_solver* s, int64_t n_total) {
  if (!s || n_total <= 0) return SGDNET_EINVAL;
  SGD_HIP_TRY(hipSetDevice(s->device));
  SGD_HIP_TRY(hipStreamSynchronize(s->st));
  s->d.n_total = (double)n_total;
  drop_graph(s);   // captured kernels carry the old value
  return SGDNET_OK;
}

int sgdnet_solver_link_peers(sgdnet_solver** solvers, int n) {
  if (!solvers || n < 1 || n > 8) {
    set_error("sgdnet_solver_link_peers: 1..8 solvers");
    return SGDNET_EINVAL;
  }
  for (int q = 0; q < n; ++q) {
    sgdnet_solver* s = solvers[q];
    if (!s || !s->d.vsync || !s->d.vx || s->d.V < 1 || s->d.V != solvers[0]->d.V || s->d.v_bps != solvers[0]->d.v_bps ||
        s->d.p != solvers[0]->d.p || s->d.K != 1) {
      set_error("sgdnet_solver_link_peers: every solver needs the same number of virtual shards (>= 2), workgroups per shard "
                "and features, and one response (rank %d does not)", q);
      return SGDNET_EUNSUPPORTED;
    }
    if (n > 1 && !vs_fused_eligible(s->d)) {
      set_error("sgdnet_solver_link_peers: the replica average across GPUs runs inside the fused epoch kernel, which rank %d's "
                "problem cannot use (sparse x, one response, an even number of features)", q);
      return SGDNET_EUNSUPPORTED;
    }
  }
  double tot = 0.0;
  for (int q = 0; q < n; ++q)
    for (int u = 0; u < solvers[q]->d.V; ++u) tot += solvers[q]->d.v_size[u];
  for (int q = 0; q < n; ++q) {
    sgdnet_solver* s = solvers[q];
    SGD_HIP_TRY(hipSetDevice(s->device));
    SGD_HIP_TRY(hipStreamSynchronize(s->st));
    drop_graph(s);
    if (n == 1) {
      s->d.peers = nullptr;
      s->d.n_peers = 0;
      continue;
    }
    for (int r = 0; r < n; ++r) {               // direct loads, stores and atomics on the other ranks' buffers
      if (solvers[r]->device == s->device) continue;
      int can = 0;
      SGD_HIP_TRY(hipDeviceCanAccessPeer(&can, s->device, solvers[r]->device));
      if (!can) {
        set_error("sgdnet_solver_link_peers: device %d cannot access device %d", s->device, solvers[r]->device);
        return SGDNET_EUNSUPPORTED;
      }
      const hipError_t e = hipDeviceEnablePeerAccess(solvers[r]->device, 0);
      if (e != hipSuccess && e != hipErrorPeerAccessAlreadyEnabled) {
        set_error("hipDeviceEnablePeerAccess(%d -> %d) failed: %s", s->device, solvers[r]->device, hipGetErrorString(e));
        return SGDNET_EHIP;
      }
      (void)hipGetLastError();
    }
    FusedPeers h{};
    h.n = n;
    h.rank = q;
    h.tot_size = tot;
    for (int r = 0; r < n; ++r) {
      h.pub[r] = solvers[r]->d.vpub;
      h.sync[r] = solvers[r]->d.vcol;
      for (int u = 0; u < 8; ++u) h.vsize[r][u] = solvers[r]->d.v_size[u];
    }
    if (!s->peers_dev) {
      void* pd = nullptr;
      SGD_HIP_TRY(hipMalloc(&pd, sizeof(FusedPeers)));
      s->owned.push_back(pd);
      s->peers_dev = static_cast<FusedPeers*>(pd);
    }
    SGD_HIP_TRY(hipMemcpy(s->peers_dev, &h, sizeof(FusedPeers), hipMemcpyHostToDevice));
    SGD_HIP_TRY(hipMemset(s->d.vsync, 0, vs_fused_sync_words() * sizeof(unsigned)));   // slice counters and launch count start together
    SGD_HIP_TRY(hipMemset(s->d.vcol, 0, vs_fused_col_words() * sizeof(unsigned)));
    s->d.peers = s->peers_dev;
    s->d.n_peers = n;
  }
  return SGDNET_OK;
}

// ---- the same link between solvers of DIFFERENT processes (one process per GPU: bench.py under torch.distributed.run) ----
// info: 2 hipIpcMemHandle_t (exchange buffer, barrier counters) + 8 shard sizes + V + workgroups per shard + features
struct PeerInfo {
  hipIpcMemHandle_t vx, vsync;
  double vsize[8];
  int V, v_bps;
  int64_t p;
};

int sgdnet_solver_peer_info_bytes(void) { return (int)sizeof(PeerInfo); }

int sgdnet_solver_peer_info(sgdnet_solver* s, void* out) {
  if (!s || !out || !s->d.vpub || !s->d.vcol) {
    set_error("sgdnet_solver_peer_info: set the virtual shards first (one response, sparse x)");
    return SGDNET_EINVAL;
  }
  SGD_HIP_TRY(hipSetDevice(s->device));
  PeerInfo h{};
  SGD_HIP_TRY(hipIpcGetMemHandle(&h.vx, s->d.vpub));
  SGD_HIP_TRY(hipIpcGetMemHandle(&h.vsync, s->d.vcol));
  for (int u = 0; u < 8; ++u) h.vsize[u] = s->d.v_size[u];
  h.V = s->d.V;
  h.v_bps = s->d.v_bps;
  h.p = s->d.p;
  memcpy(out, &h, sizeof(h));
  return SGDNET_OK;
}

int sgdnet_solver_link_ipc(sgdnet_solver* s, int rank, int n, const void* infos) {
  if (!s || !infos || n < 2 || n > 8 || rank < 0 || rank >= n) {
    set_error("sgdnet_solver_link_ipc: 2..8 ranks");
    return SGDNET_EINVAL;
  }
  SGD_HIP_TRY(hipSetDevice(s->device));
  SGD_HIP_TRY(hipStreamSynchronize(s->st));
  if (!vs_fused_eligible(s->d)) {
    set_error("sgdnet_solver_link_ipc: the replica average across GPUs runs inside the fused epoch kernel, which this "
              "problem cannot use (sparse x, one response, an even number of features, virtual shards set)");
    return SGDNET_EUNSUPPORTED;
  }
  const PeerInfo* I = static_cast<const PeerInfo*>(infos);
  FusedPeers h{};
  h.n = n;
  h.rank = rank;
  for (int r = 0; r < n; ++r) {
    if (I[r].V != s->d.V || I[r].v_bps != s->d.v_bps || I[r].p != s->d.p) {
      set_error("sgdnet_solver_link_ipc: rank %d has %d shards of %d workgroups on %lld features, this rank %d of %d on %lld",
                r, I[r].V, I[r].v_bps, (long long)I[r].p, s->d.V, s->d.v_bps, (long long)s->d.p);
      return SGDNET_EUNSUPPORTED;
    }
    for (int u = 0; u < 8; ++u) {
      h.vsize[r][u] = I[r].vsize[u];
      if (u < I[r].V) h.tot_size += I[r].vsize[u];
    }
    if (r == rank) {
      h.pub[r] = s->d.vpub;
      h.sync[r] = s->d.vcol;
    } else {
      void *px = nullptr, *py = nullptr;
      SGD_HIP_TRY(hipIpcOpenMemHandle(&px, I[r].vx, hipIpcMemLazyEnablePeerAccess));
      SGD_HIP_TRY(hipIpcOpenMemHandle(&py, I[r].vsync, hipIpcMemLazyEnablePeerAccess));
      s->ipc_opened.push_back(px);
      s->ipc_opened.push_back(py);
      h.pub[r] = static_cast<double*>(px);
      h.sync[r] = static_cast<unsigned*>(py);
    }
  }
  drop_graph(s);
  if (!s->peers_dev) {
    void* pd = nullptr;
    SGD_HIP_TRY(hipMalloc(&pd, sizeof(FusedPeers)));
    s->owned.push_back(pd);
    s->peers_dev = static_cast<FusedPeers*>(pd);
  }
  SGD_HIP_TRY(hipMemcpy(s->peers_dev, &h, sizeof(FusedPeers), hipMemcpyHostToDevice));
  // (the counters were zeroed when the shards were set; every rank links before any of them enqueues an epoch -- the
  //  caller's barrier -- so nothing is cleared here that a peer may already have added to)
  s->d.peers = s->peers_dev;
  s->d.n_peers = n;
  return SGDNET_OK;
}

}  // extern "C"
