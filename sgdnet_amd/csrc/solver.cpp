// Device-resident SAGA solver behind the sgdnet_solver_* C ABI (include/sgdnet_hip.h): life cycle and data.
//
// Owns the HBM copies of the sample-major data and of the five state arrays the
// reference keeps alive along the lambda path (src/sgdnet.cpp:187-198): create / destroy, the packed records,
// the scratch of the binned and tiled forms, where the gradient memory lives, penalty, state access, deviance
// and the deltas of the multi-GPU merge.  Also the error string and the option table.  The epochs themselves are
// solver_epoch.cpp's, the sample stream solver_rng.cpp's, shards and links solver_shards.cpp's (solver_state.hpp).
#include <math.h>
#include <stdarg.h>
#include <stdlib.h>
#include <stdio.h>
#include <string.h>

#include <algorithm>
#include <string>
#include <atomic>
#include <vector>

#include <hip/hip_ext.h>

#include "solver_state.hpp"

namespace sgdnet {

static thread_local std::string g_last_error;

void set_error(const char* fmt, ...) {
  char buf[1024];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof(buf), fmt, ap);
  va_end(ap);
  g_last_error = buf;
}

template <typename T>
static int dev_alloc(sgdnet_solver* s, T** out, size_t count, bool zero) {
  void* p = nullptr;
  const size_t bytes = sizeof(T) * (count ? count : 1);
  hipError_t e = hipMalloc(&p, bytes);
  if (e != hipSuccess) {
    set_error("hipMalloc(%zu bytes) failed: %s", bytes, hipGetErrorString(e));
    return SGDNET_ENOMEM;
  }
  s->owned.push_back(p);
  if (zero) SGD_HIP_TRY(hipMemsetAsync(p, 0, bytes, s->st));
  *out = static_cast<T*>(p);
  return SGDNET_OK;
}

template <typename T>
static int dev_upload(sgdnet_solver* s, T** out, const T* host, size_t count) {
  int rc = dev_alloc(s, out, count, false);
  if (rc) return rc;
  if (count) SGD_HIP_TRY(hipMemcpyAsync(*out, host, sizeof(T) * count, hipMemcpyHostToDevice, s->st));
  return SGDNET_OK;
}

// Where the gradient memory of a one-response sparse fit lives: inside the compact records while batched
// epochs run (the gather reads it with the record and stores it back in place), in the K x n array for the
// exact kernels and the host.  A move is one pass over the samples; it happens when the mode changes or the
// host reads / writes g_memory, not per epoch.  The kernels take SagaDev by value, so captured graphs go.
int m_to_record(sgdnet_solver* s) {
  if (s->m_in_rec || !s->d.cP || s->d.K != 1) return SGDNET_OK;
  int rc = launch_m_move(s->d, 1, s->st);
  if (rc) return rc;
  s->m_in_rec = true;
  s->d.m_rec = 1;
  s->d.m_base = s->d.cP + 120;
  s->d.m_stride = 128;
  drop_graph(s);
  return SGDNET_OK;
}

int m_to_array(sgdnet_solver* s) {
  if (!s->m_in_rec) return SGDNET_OK;
  int rc = launch_m_move(s->d, 0, s->st);
  if (rc) return rc;
  s->m_in_rec = false;
  s->d.m_rec = 0;
  s->d.m_base = reinterpret_cast<char*>(s->d.M);
  s->d.m_stride = 8;
  drop_graph(s);
  return SGDNET_OK;
}

// Binned form of the batched iteration for K x p tables that fit no LDS (batched_binned.hip
// "Binned form").  Ranges: contiguous features of equal non-zero mass, at most
// binned_max_range_features(K) wide; built once per solver from a device histogram of the feature
// ids.  Bins and the gradient-change buffer are sized for the batch.
int ensure_binned(sgdnet_solver* s, int64_t batch) {
  SagaDev& d = s->d;
  if (s->bin_disabled || !wants_binned(d, batch)) {
    if (d.R > 0 && d.bins) {             // e.g. a tiny batch after a large one: fall back to the atomic form
      d.bins = nullptr;
      drop_graph(s);
    }
    return SGDNET_OK;
  }
  if (!s->bin_ranges_ready) {
    s->bin_ranges_ready = true;                       // whatever comes out: the work below is done once
    unsigned* counts = nullptr;
    SGD_HIP_TRY(hipMalloc(reinterpret_cast<void**>(&counts), sizeof(unsigned) * (size_t)d.p));
    struct Free { void* q; ~Free() { (void)hipFree(q); } } free_counts{counts};
    int rc = launch_col_count(d, s->nnz, counts, s->st);
    if (rc) return rc;
    std::vector<unsigned> h((size_t)d.p);
    SGD_HIP_TRY(hipMemcpyAsync(h.data(), counts, sizeof(unsigned) * h.size(), hipMemcpyDeviceToHost, s->st));
    SGD_HIP_TRY(hipStreamSynchronize(s->st));
    const int64_t fmax = (int64_t)binned_max_range_features(d.K);
    static const int target_env = exp_env_int("SGDNET_BIN_RANGES", 0);
    // range sweep workgroups: two of them fit a CU beside each other (64 KB of LDS each at the widest range), and the
    // launch carries one more workgroup for the intercept -- 2 x 256 - 12 ranges keep the whole launch resident in one
    // wave (round 4: the rule's rounding made 513 ranges + 1 of 512, the last two workgroups ran after everybody else)
    const int target = target_env > 0 ? target_env : 500;
    const double per = std::max(1.0, (double)s->nnz / target);
    std::vector<int32_t> lo{0};
    {
      double mass = 0.0;
      int64_t width = 0;
      for (int64_t j = 0; j < d.p; ++j) {
        if (width > 0 && (width >= fmax || mass + 0.5 * h[(size_t)j] >= per)) {
          lo.push_back((int32_t)j);
          mass = 0.0;
          width = 0;
        }
        mass += h[(size_t)j];
        ++width;
      }
      lo.push_back((int32_t)d.p);
    }
    const int R = (int)lo.size() - 1;
    if (R > 2048) return SGDNET_OK;      // staging counters of the gather would not fit: d.R stays 0 (no binned form)
    std::vector<uint16_t> fr((size_t)d.p);
    s->bin_mass.assign((size_t)R, 0.0);
    int wmax = 1;
    for (int r = 0; r < R; ++r) {
      wmax = std::max(wmax, (int)(lo[(size_t)r + 1] - lo[(size_t)r]));
      for (int64_t j = lo[(size_t)r]; j < lo[(size_t)r + 1]; ++j) {
        fr[(size_t)j] = (uint16_t)r;
        s->bin_mass[(size_t)r] += h[(size_t)j];
      }
    }
    d.range_max = wmax;
    int32_t* lo_dev = nullptr;
    uint16_t* fr_dev = nullptr;
    uint16_t* rc_dev = nullptr;
    // coarse cells of 2^shift features (at most 2047 of them): the range of a cell's first feature
    int shift = 7;
    while (((d.p + (1ll << shift) - 1) >> shift) + 1 > 2048) ++shift;
    const int n_coarse = (int)((d.p + (1ll << shift) - 1) >> shift);
    std::vector<uint16_t> rcv((size_t)n_coarse + 1);
    for (int c = 0; c < n_coarse; ++c) rcv[(size_t)c] = fr[(size_t)c << shift];
    rcv[(size_t)n_coarse] = (uint16_t)(R - 1);
    rc = dev_upload(s, &lo_dev, lo.data(), lo.size());
    if (!rc) rc = dev_upload(s, &fr_dev, fr.data(), fr.size());
    if (!rc) rc = dev_upload(s, &rc_dev, rcv.data(), rcv.size());
    unsigned* bc = nullptr;
    int* be = nullptr;
    if (!rc) rc = dev_alloc(s, &bc, (size_t)R, true);
    if (!rc) rc = dev_alloc(s, &be, 1, true);
    if (rc) return rc;
    // second moment of a sample's entries per range (sizes the bins below)
    s->bin_sumsq.assign((size_t)R, 0.0);
    if (d.ptr) {
      unsigned long long* sq = nullptr;
      SGD_HIP_TRY(hipMalloc(reinterpret_cast<void**>(&sq), sizeof(unsigned long long) * (size_t)R));
      Free free_sq{sq};
      rc = launch_range_moment(d, fr_dev, sq, R, s->st);
      if (rc) return rc;
      std::vector<unsigned long long> hsq((size_t)R);
      SGD_HIP_TRY(hipMemcpyAsync(hsq.data(), sq, sizeof(unsigned long long) * (size_t)R, hipMemcpyDeviceToHost, s->st));
      SGD_HIP_TRY(hipStreamSynchronize(s->st));
      for (int r = 0; r < R; ++r) s->bin_sumsq[(size_t)r] = (double)hsq[(size_t)r];
    } else {
      s->bin_sumsq = s->bin_mass;                     // no sample-major pointers: one entry per arrival
    }
    SGD_HIP_TRY(hipStreamSynchronize(s->st));        // the uploads read host vectors that die here
    int ks = 1;
    while (ks < d.K) ks *= 2;
    d.KS = ks;
    if (ks != d.K) {
      double* wp = nullptr;
      rc = dev_alloc(s, &wp, (size_t)d.p * (size_t)ks, true);
      if (rc) return rc;
      d.wpad = wp;
    } else {
      d.wpad = d.w;
    }
    d.R = R;
    d.range_lo = lo_dev;
    d.feat_range = fr_dev;
    d.range_coarse = rc_dev;
    d.coarse_shift = shift;
    d.n_coarse = n_coarse;
    d.bin_count = bc;
    d.bin_err = be;
    if (getenv("SGDNET_TRACE")) fprintf(stderr, "[sgdnet]   binned form: %d feature ranges (<= %lld features each)\n", R, (long long)fmax);
  }
  if (d.R <= 0) return SGDNET_OK;
  if (batch != s->bin_batch || !s->bin_bufs[0] || s->bin_slack != s->bin_slack_built) {
    SGD_HIP_TRY(hipStreamSynchronize(s->st));
    for (void*& q : s->bin_bufs) {
      if (q) (void)hipFree(q);
      q = nullptr;
    }
    // Range r receives the entries of `batch` uniformly drawn samples: a sum of `batch` per-sample counts c_ir
    // with mean mass_r / n and second moment sumsq_r / n.  Capacity = mean + slack standard deviations + room
    // for the largest rows (slack starts at 8 and doubles when a bin has overflowed: solver_grow_bins).
    std::vector<int64_t> off((size_t)d.R + 1, 0);
    for (int r = 0; r < d.R; ++r) {
      const double mean = (double)batch * s->bin_mass[(size_t)r] / (double)d.n;
      const double var = (double)batch * s->bin_sumsq[(size_t)r] / (double)d.n;
      double cap = mean + s->bin_slack * std::sqrt(var) + 64.0 * s->bin_slack;
      cap = std::min(cap, (double)batch * (double)d.range_max + 512.0);   // nothing can send more than this
      off[(size_t)r + 1] = off[(size_t)r] + (int64_t)cap;
    }
    SGD_HIP_TRY(hipMalloc(&s->bin_bufs[0], (size_t)16 * (size_t)off[(size_t)d.R]));
    SGD_HIP_TRY(hipMalloc(&s->bin_bufs[1], sizeof(double) * (size_t)batch * (size_t)d.KS));
    SGD_HIP_TRY(hipMalloc(&s->bin_bufs[2], sizeof(int64_t) * off.size()));
    SGD_HIP_TRY(hipMemcpy(s->bin_bufs[2], off.data(), sizeof(int64_t) * off.size(), hipMemcpyHostToDevice));
    s->bin_batch = batch;
    s->bin_slack_built = s->bin_slack;
    drop_graph(s);
  }
  if (!d.bins) drop_graph(s);
  d.bins = static_cast<char*>(s->bin_bufs[0]);
  d.gcb = static_cast<double*>(s->bin_bufs[1]);
  d.bin_off = static_cast<const int64_t*>(s->bin_bufs[2]);
  return SGDNET_OK;
}

// Dense x whose K x p accumulator fits no LDS (batched_dense.hip "tiled"): the gather leaves the
// batch's gradient changes in d.gcb and D is formed feature tile by feature tile.
int ensure_dense_tiled(sgdnet_solver* s, int64_t batch) {
  SagaDev& d = s->d;
  if (!wants_tiles(d)) return SGDNET_OK;
  if (batch > s->bin_batch || !s->bin_bufs[1]) {
    SGD_HIP_TRY(hipStreamSynchronize(s->st));
    if (s->bin_bufs[1]) (void)hipFree(s->bin_bufs[1]);
    s->bin_bufs[1] = nullptr;
    SGD_HIP_TRY(hipMalloc(&s->bin_bufs[1], sizeof(double) * (size_t)batch * (size_t)d.K));
    s->bin_batch = batch;
    drop_graph(s);
  }
  d.gcb = static_cast<double*>(s->bin_bufs[1]);
  d.KS = d.K;
  return SGDNET_OK;
}

// Packs the sample-major CSR rows into fixed-stride records for the batched gather
// (layout: batched_device.hpp "Packed sample records").
constexpr int kOvfStride = 256;
constexpr int kOvfCap = 20;

static int build_records(sgdnet_solver* s, const sgdnet_problem* pb) {
  const int64_t n = pb->n_samples;
  SagaDev& d = s->d;
  // capacity: 90th percentile of the row lengths (histogram; rows rarely exceed a few hundred)
  std::vector<int64_t> hist(65, 0);
  int64_t zmax = 0;
  for (int64_t i = 0; i < n; ++i) {
    const int64_t z = pb->rowptr[i + 1] - pb->rowptr[i];
    hist[(size_t)(z < 64 ? z : 64)]++;
    zmax = z > zmax ? z : zmax;
  }
  int cap = 1;
  {
    int64_t acc = 0;
    const int64_t want = (int64_t)(0.9 * (double)n);
    for (int z = 0; z <= 64; ++z) {
      acc += hist[(size_t)z];
      cap = z < 1 ? 1 : z;
      if (acc >= want) break;
    }
    if (cap >= 64) cap = (int)(zmax < 512 ? zmax : 512);
  }
  auto rec_bytes = [](int c) { return 16 + ((4 * c + 7) & ~7) + 8 * c; };
  // records are aligned to 128 B: random HBM requests on gfx950 are served in 128-B units
  // (measured: 64-B-aligned 192-B records cost 13 % more gather time than 256-B ones)
  static const int align = exp_env_int("SGDNET_REC_ALIGN", 128);
  const int stride = (rec_bytes(cap) + align - 1) / align * align;
  while (rec_bytes(cap + 1) <= stride) ++cap;
  const int val_off = 16 + ((4 * cap + 7) & ~7);
  if ((double)n * stride > 64e9) {
    set_error("packed records would need %.1f GB", (double)n * stride / 1e9);
    return SGDNET_ENOMEM;
  }
  std::vector<char> rec((size_t)n * (size_t)stride, 0);
  std::vector<char> ovf;
  const bool y_in_rec = pb->y_rows == 1;
  for (int64_t i = 0; i < n; ++i) {
    char* base = rec.data() + (size_t)i * (size_t)stride;
    const int64_t q0 = pb->rowptr[i];
    const int nnz = (int)(pb->rowptr[i + 1] - q0);
    const double y0 = y_in_rec ? pb->y[i] : 0.0;
    memcpy(base, &y0, 8);
    memcpy(base + 8, &nnz, 4);
    const int c0 = nnz < cap ? nnz : cap;
    memcpy(base + 16, pb->colidx + q0, sizeof(int32_t) * (size_t)c0);
    memcpy(base + val_off, pb->values + q0, sizeof(double) * (size_t)c0);
    int done = c0;
    int32_t* link = reinterpret_cast<int32_t*>(base + 12);   // where the next record's index goes
    size_t link_off = (size_t)(reinterpret_cast<char*>(link) - rec.data());
    bool link_in_rec = true;
    while (done < nnz) {
      const int c = (nnz - done) < kOvfCap ? (nnz - done) : kOvfCap;
      const int32_t id = (int32_t)(ovf.size() / kOvfStride);
      ovf.resize(ovf.size() + kOvfStride, 0);
      char* ob = ovf.data() + (size_t)id * kOvfStride;
      memcpy(ob + 4, &c, 4);
      memcpy(ob + 8, pb->colidx + q0 + done, sizeof(int32_t) * (size_t)c);
      memcpy(ob + 8 + 4 * kOvfCap, pb->values + q0 + done, sizeof(double) * (size_t)c);
      // patch the previous link (vectors may have been reallocated: use offsets)
      if (link_in_rec) memcpy(rec.data() + link_off, &id, 4);
      else memcpy(ovf.data() + link_off, &id, 4);
      link_off = (size_t)id * kOvfStride;
      link_in_rec = false;
      done += c;
    }
  }
  char* rec_dev = nullptr;
  char* ovf_dev = nullptr;
  int rc = dev_upload(s, &rec_dev, rec.data(), rec.size());
  if (rc) return rc;
  rc = dev_upload(s, &ovf_dev, ovf.data(), ovf.size());
  if (rc) return rc;
  SGD_HIP_TRY(hipStreamSynchronize(s->st));   // host vectors die at return
  d.rec = rec_dev;
  d.ovf = ovf_dev;
  d.rec_stride = stride;
  d.rec_cap = cap;
  d.rec_val_off = val_off;
  return SGDNET_OK;
}

}  // namespace sgdnet

using namespace sgdnet;

namespace {
struct OptionDef {
  const char* name;
  int dflt, lo, hi;
};
const OptionDef kOptionDefs[sgdnet::kOptCount] = {
    {"virtual_shards", -1, -1, 8}, {"rng_generators", 0, 0, 64},     {"window_eigenvalue", 1, 0, 1},
    {"host_setup", 0, 0, 1},       {"exact_epoch_blocks", 1, 0, 1}, {"exact_row_registers", 1, 0, 4},
    {"fused_epoch", 1, 0, 2},      {"wcovariance_width", 0, 0, 1024}, {"wnewton_width", 0, 0, 1024},
    {"wmcovariance_width", 0, 0, 1024}, {"wmnewton_width", 0, 0, 1024},
};
std::atomic<int> g_options[sgdnet::kOptCount] = {{-1}, {0}, {1}, {0}, {1}, {1}, {1}, {0}, {0}, {0}, {0}};
int find_option(const char* name) {
  if (name)
    for (int i = 0; i < sgdnet::kOptCount; ++i)
      if (!strcmp(name, kOptionDefs[i].name)) return i;
  return -1;
}
}  // namespace

namespace sgdnet {
int option(Option o) { return g_options[o].load(std::memory_order_relaxed); }
}  // namespace sgdnet

extern "C" {

int sgdnet_abi_version(void) { return SGDNET_ABI_VERSION; }

int sgdnet_set_option(const char* name, int value) {
  const int i = find_option(name);
  if (i < 0 || value < kOptionDefs[i].lo || value > kOptionDefs[i].hi) {
    set_error("sgdnet_set_option: %s = %d is not an option (include/sgdnet_hip.h)", name ? name : "(null)", value);
    return SGDNET_EINVAL;
  }
  g_options[i].store(value, std::memory_order_relaxed);
  return SGDNET_OK;
}

int sgdnet_get_option(const char* name, int* value) {
  const int i = find_option(name);
  if (i < 0 || !value) {
    set_error("sgdnet_get_option: unknown option %s", name ? name : "(null)");
    return SGDNET_EINVAL;
  }
  *value = g_options[i].load(std::memory_order_relaxed);
  return SGDNET_OK;
}

const char* sgdnet_last_error(void) { return g_last_error.c_str(); }

int sgdnet_device_count(void) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) return 0;
  return n;
}

extern "C" void sgdnet_solver_destroy(sgdnet_solver* s);

static int solver_create_impl(const sgdnet_problem* pb, DeviceSetup* adopt, sgdnet_solver** out) {
  if (!pb || !out) {
    set_error("sgdnet_solver_create: null argument");
    return SGDNET_EINVAL;
  }
  *out = nullptr;
  if (pb->n_samples <= 0 || pb->n_features <= 0 || pb->n_classes <= 0 || !pb->y || pb->y_rows <= 0 ||
      (!adopt && !pb->x_dense && !(pb->rowptr && pb->colidx && pb->values))) {
    set_error("sgdnet_solver_create: invalid problem description");
    return SGDNET_EINVAL;
  }
  if (pb->family < SGDNET_GAUSSIAN || pb->family > SGDNET_MGAUSSIAN) {
    set_error("sgdnet_solver_create: unknown family %d", pb->family);
    return SGDNET_EINVAL;
  }
  if (pb->n_samples > 0xFFFFFFFFll) {
    set_error("sgdnet_solver_create: n_samples exceeds the reference's unsigned range");
    return SGDNET_EINVAL;
  }
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) {
    set_error("no HIP device available: the SAGA backend has no CPU fallback");
    return SGDNET_ENODEVICE;
  }
  if (pb->device < 0 || pb->device >= ndev) {
    set_error("device %d out of range (%d devices)", pb->device, ndev);
    return SGDNET_EINVAL;
  }
  SGD_HIP_TRY(hipSetDevice(pb->device));

  sgdnet_solver* s = new sgdnet_solver();
  s->device = pb->device;
  (void)hipDeviceGetAttribute(&s->cus, hipDeviceAttributeMultiprocessorCount, s->device);
  s->sparse = adopt ? adopt->xd_t == nullptr : pb->x_dense == nullptr;
  hipError_t e = hipStreamCreateWithFlags(&s->st, hipStreamNonBlocking);
  if (e != hipSuccess) {
    set_error("hipStreamCreate failed: %s", hipGetErrorString(e));
    delete s;
    return SGDNET_EHIP;
  }
  SagaDev& d = s->d;
  d.family = pb->family;
  d.K = pb->n_classes;
  d.Ky = pb->y_rows;
  d.fit_intercept = pb->fit_intercept;
  d.standardize = (s->sparse && pb->standardize && (adopt || pb->x_center_scaled)) ? 1 : 0;
  d.n = pb->n_samples;
  d.p = pb->n_features;
  d.n_total = (double)(pb->n_total > 0 ? pb->n_total : pb->n_samples);
#ifdef SGDNET_EXPERIMENTS
  d.ablate = getenv("SGDNET_ABLATE") ? atoi(getenv("SGDNET_ABLATE")) : 0;
#else
  d.ablate = 0;
#endif
#ifdef SGDNET_PHASE_TIMING
  if (hipMalloc(&d.dbg, sizeof(unsigned long long) * 16 * 4096) != hipSuccess) d.dbg = nullptr;
  if (d.dbg) (void)hipMemset(d.dbg, 0, sizeof(unsigned long long) * 16 * 4096);
#endif

  const size_t n = (size_t)d.n, p = (size_t)d.p, K = (size_t)d.K;
  int rc = SGDNET_OK;
#define TRY(x)                     \
  do {                             \
    rc = (x);                      \
    if (rc) {                      \
      sgdnet_solver_destroy(s);    \
      return rc;                   \
    }                              \
  } while (0)
  if (adopt && adopt->xd_t) {
    // dense x standardised and transposed on the device (dense_setup_*): take ownership
    s->nnz = (int64_t)n * (int64_t)p;
    d.xd = adopt->xd_t;
    s->owned.push_back(adopt->xd_t);
    adopt->xd_t = nullptr;
  } else if (adopt) {
    // buffers produced on the device by setup_device.hip: take ownership
    s->nnz = adopt->nnz;
    d.avg_nnz = adopt->avg_nnz;
    d.ptr = adopt->sptr;
    d.idx = adopt->sidx;
    d.val = adopt->sval;
    d.rec = adopt->rec;
    d.ovf = adopt->ovf;
    d.rec_stride = adopt->rec_stride;
    d.rec_cap = adopt->rec_cap;
    d.rec_val_off = adopt->rec_val_off;
    for (void* q : {(void*)adopt->sptr, (void*)adopt->sidx, (void*)adopt->sval, (void*)adopt->rec,
                    (void*)adopt->ovf})
      s->owned.push_back(q);
    adopt->sptr = nullptr;
    adopt->sidx = nullptr;
    adopt->sval = nullptr;
    adopt->rec = adopt->ovf = nullptr;
    if (d.standardize) {
      d.c = adopt->center_scaled;
      s->owned.push_back(adopt->center_scaled);
      adopt->center_scaled = nullptr;
    }
  } else if (s->sparse) {
    s->nnz = pb->rowptr[n];
    d.avg_nnz = (float)((double)s->nnz / (double)n);
    int64_t* ptr;
    int32_t* idx;
    double* val;
    TRY(dev_upload(s, &ptr, pb->rowptr, n + 1));
    TRY(dev_upload(s, &idx, pb->colidx, (size_t)s->nnz));
    TRY(dev_upload(s, &val, pb->values, (size_t)s->nnz));
    d.ptr = ptr;
    d.idx = idx;
    d.val = val;
    TRY(build_records(s, pb));
  } else {
    double* xd;
    TRY(dev_upload(s, &xd, pb->x_dense, n * p));
    d.xd = xd;
  }
  {
    double* y;
    TRY(dev_upload(s, &y, pb->y, n * (size_t)d.Ky));
    d.y = y;
    if (d.standardize && !adopt) {
      double* c;
      TRY(dev_upload(s, &c, pb->x_center_scaled, p));
      d.c = c;
    }
  }
  d.y_binary = 0;
  if (d.family == SGDNET_BINOMIAL) {
    d.y_binary = 1;
    for (size_t i = 0; i < n * (size_t)d.Ky; ++i)
      if (pb->y[i] != 0.0 && pb->y[i] != 1.0) {
        d.y_binary = 0;
        break;
      }
  }
  if (s->sparse && compact_eligible(d)) {
    // an optimisation, not a requirement: without the memory for the planes the K = 1 gather
    // reads the 256-B records
    char *cP = nullptr, *cQ = nullptr;
    uint32_t* mt = nullptr;
    if (dev_alloc(s, &cP, (n + 1) * 128, false) == SGDNET_OK && dev_alloc(s, &cQ, (n + 1) * 128, false) == SGDNET_OK &&
        dev_alloc(s, &mt, (n + 15) / 16 + 1, false) == SGDNET_OK) {
      TRY(launch_pack_compact(d, cP, cQ, mt, s->st));
      d.cP = cP;
      d.cQ = cQ;
      d.cmeta = mt;
      d.cE = compact_entries(d);
    } else {
      (void)hipGetLastError();
    }
  }
  TRY(dev_alloc(s, &d.w, K * p, true));
  TRY(dev_alloc(s, &d.G, K * p, true));
  TRY(dev_alloc(s, &d.M, K * n, true));
  d.m_base = reinterpret_cast<char*>(d.M);
  d.m_stride = 8;
  TRY(dev_alloc(s, &d.b, K, true));
  TRY(dev_alloc(s, &d.gb, K, true));
  TRY(dev_alloc(s, &d.w_prev, K * p, true));
  TRY(dev_alloc(s, &d.lag, p, true));
  TRY(dev_alloc(s, &d.D, K * p, true));
  TRY(dev_alloc(s, &d.claim, n, false));
  TRY(dev_alloc(s, &d.d0_part, 2 * 256 * K, true));   // two parity sets of 256 slots (batched_geometry.hpp: kD0Slots)
  TRY(dev_alloc(s, &d.cw, 2 * 16 * K, true));
  TRY(dev_alloc(s, &s->ref, 2 * K * p + 2 * K, true));
  TRY(dev_alloc(s, &s->out_dev, 4, true));
  TRY(dev_alloc(s, &s->lam_dev, 1, true));
#undef TRY
  e = hipHostMalloc(reinterpret_cast<void**>(&s->lam_stage), sizeof(LamParams) * sgdnet_solver::kLamSlots,
                    hipHostMallocDefault);
  for (int i = 0; e == hipSuccess && i < sgdnet_solver::kLamSlots; ++i)
    e = hipEventCreateWithFlags(&s->lam_ev[i], hipEventDisableTiming);
  if (e != hipSuccess) {
    set_error("solver initialisation failed: %s", hipGetErrorString(e));
    sgdnet_solver_destroy(s);
    return SGDNET_EHIP;
  }
  e = hipMemsetAsync(d.claim, 0xFF, sizeof(int) * n, s->st);  // -1: never a batch id
  if (e == hipSuccess) e = hipStreamSynchronize(s->st);
  if (e != hipSuccess) {
    set_error("solver initialisation failed: %s", hipGetErrorString(e));
    sgdnet_solver_destroy(s);
    return SGDNET_EHIP;
  }
  memset(&s->lam, 0, sizeof(s->lam));
  *out = s;
  return SGDNET_OK;
}

int sgdnet_solver_create(const sgdnet_problem* pb, sgdnet_solver** out) {
  return solver_create_impl(pb, nullptr, out);
}

void sgdnet_solver_destroy(sgdnet_solver* s) {
  if (!s) return;
  if (getenv("SGDNET_TRACE") && s->trace_epochs) {
    fprintf(stderr, "[sgdnet]   batched epochs %ld: graph launch calls %.3f s, waiting for the epoch + ConvergenceCheck %.3f s, epoch graphs on the device %.3f s\n",
            s->trace_epochs, s->trace_launch, s->trace_conv, s->trace_graph);
  }
  (void)hipSetDevice(s->device);
  if (s->st) (void)hipStreamSynchronize(s->st);
  drop_graph(s);
  for (void* q : s->ipc_opened) (void)hipIpcCloseMemHandle(q);
  for (hipEvent_t e : s->epoch_ev) (void)hipEventDestroy(e);
  for (hipEvent_t e : s->ev_pool) (void)hipEventDestroy(e);
  for (hipEvent_t e : s->trace_ev)
    if (e) (void)hipEventDestroy(e);
  for (void* p : s->owned) (void)hipFree(p);
  if (s->LS_dev) (void)hipFree(s->LS_dev);
  if (s->d.slab) (void)hipFree(s->d.slab);
  for (void* q : s->bin_bufs)
    if (q) (void)hipFree(q);
  for (void* q : s->vs_owned) (void)hipFree(q);
  if (s->lam_stage) (void)hipHostFree(s->lam_stage);
  for (hipEvent_t ev : s->lam_ev)
    if (ev) (void)hipEventDestroy(ev);
  if (s->stream_dev) (void)hipFree(s->stream_dev);
  if (s->rng_dev) (void)hipFree(s->rng_dev);
  if (s->pipe.st) {
    (void)hipStreamSynchronize(s->pipe.st);
    (void)hipStreamDestroy(s->pipe.st);
  }
  for (int i = 0; i < 2; ++i) {
    if (s->pipe.ready[i]) (void)hipEventDestroy(s->pipe.ready[i]);
    if (s->pipe.freed[i]) (void)hipEventDestroy(s->pipe.freed[i]);
    if (s->pipe.state[i]) (void)hipFree(s->pipe.state[i]);
  }
  if (s->pipe.poly_n) (void)hipFree(s->pipe.poly_n);
  if (s->pipe.dev) (void)hipFree(s->pipe.dev);
  if (s->pipe.ends) (void)hipFree(s->pipe.ends);
  if (s->st) (void)hipStreamDestroy(s->st);
  delete s;
}

int sgdnet_solver_set_penalty(sgdnet_solver* s, int penalty, double gamma, double alpha, double beta) {
  if (!s || penalty < SGDNET_RIDGE || penalty > SGDNET_GROUPLASSO || !(gamma > 0.0)) {
    set_error("sgdnet_solver_set_penalty: invalid argument");
    return SGDNET_EINVAL;
  }
  SGD_HIP_TRY(hipSetDevice(s->device));
  if (penalty != s->lam.penalty) drop_graph(s);   // the captured sweep kernel depends on it
  s->lam.penalty = penalty;
  s->lam.gamma = gamma;
  s->lam.alpha = alpha;
  s->lam.beta = beta;
  s->penalty_set = true;
  return push_lam(s);
}

static int state_ptr(sgdnet_solver* s, int which, double** p, size_t* count) {
  const size_t K = (size_t)s->d.K, n = (size_t)s->d.n, pp = (size_t)s->d.p;
  switch (which) {
    case 0: *p = s->d.w; *count = K * pp; break;
    case 1: *p = s->d.b; *count = K; break;
    case 2: *p = s->d.M; *count = K * n; break;
    case 3: *p = s->d.G; *count = K * pp; break;
    case 4: *p = s->d.gb; *count = K; break;
    default:
      set_error("unknown state array %d", which);
      return SGDNET_EINVAL;
  }
  return SGDNET_OK;
}

int sgdnet_solver_get_state(sgdnet_solver* s, int which, double* host) {
  if (!s || !host) return SGDNET_EINVAL;
  SGD_HIP_TRY(hipSetDevice(s->device));
  double* p;
  size_t count;
  int rc = state_ptr(s, which, &p, &count);
  if (rc) return rc;
  if (which == 2) rc = m_to_array(s);
  if (rc) return rc;
  SGD_HIP_TRY(hipMemcpyAsync(host, p, sizeof(double) * count, hipMemcpyDeviceToHost, s->st));
  SGD_HIP_TRY(hipStreamSynchronize(s->st));
  return SGDNET_OK;
}

int sgdnet_solver_set_state(sgdnet_solver* s, int which, const double* host) {
  if (!s || !host) return SGDNET_EINVAL;
  SGD_HIP_TRY(hipSetDevice(s->device));
  double* p;
  size_t count;
  int rc = state_ptr(s, which, &p, &count);
  if (rc) return rc;
  if (which == 2) rc = m_to_array(s);
  if (rc) return rc;
  SGD_HIP_TRY(hipMemcpyAsync(p, host, sizeof(double) * count, hipMemcpyHostToDevice, s->st));
  SGD_HIP_TRY(hipStreamSynchronize(s->st));
  if (which == 0) s->w_prev_valid = false;
  return SGDNET_OK;
}

int sgdnet_solver_deviance(sgdnet_solver* s, double* out) {
  if (!s || !out) return SGDNET_EINVAL;
  SGD_HIP_TRY(hipSetDevice(s->device));
  double sum = 0.0;
  int rc = device_loss_sum(s, &sum);
  if (rc) return rc;
  *out = 2.0 * sum;
  return SGDNET_OK;
}

int64_t sgdnet_solver_delta_len(const sgdnet_solver* s) {
  if (!s) return 0;
  return 2 * (int64_t)s->d.K * s->d.p + 2 * s->d.K;
}

int sgdnet_solver_snapshot(sgdnet_solver* s) {
  if (!s) return SGDNET_EINVAL;
  SGD_HIP_TRY(hipSetDevice(s->device));
  const size_t KP = (size_t)s->d.K * (size_t)s->d.p, K = (size_t)s->d.K;
  SGD_HIP_TRY(hipMemcpyAsync(s->ref, s->d.G, 8 * KP, hipMemcpyDeviceToDevice, s->st));
  SGD_HIP_TRY(hipMemcpyAsync(s->ref + KP, s->d.w, 8 * KP, hipMemcpyDeviceToDevice, s->st));
  SGD_HIP_TRY(hipMemcpyAsync(s->ref + 2 * KP, s->d.gb, 8 * K, hipMemcpyDeviceToDevice, s->st));
  SGD_HIP_TRY(hipMemcpyAsync(s->ref + 2 * KP + K, s->d.b, 8 * K, hipMemcpyDeviceToDevice, s->st));
  return SGDNET_OK;
}

void* sgdnet_solver_stream(sgdnet_solver* s) { return s ? static_cast<void*>(s->st) : nullptr; }

int sgdnet_solver_export_delta_weighted_async(sgdnet_solver* s, void* device_buf, double weight) {
  if (!s || !device_buf) return SGDNET_EINVAL;
  SGD_HIP_TRY(hipSetDevice(s->device));
  return launch_delta_export(s->d, s->ref, static_cast<double*>(device_buf), weight, s->st);
}

int sgdnet_solver_export_delta_async(sgdnet_solver* s, void* device_buf) {
  return sgdnet_solver_export_delta_weighted_async(s, device_buf, 1.0);
}

int sgdnet_solver_apply_merged_async(sgdnet_solver* s, const void* device_buf, double w_weight) {
  if (!s || !device_buf) return SGDNET_EINVAL;
  SGD_HIP_TRY(hipSetDevice(s->device));
  return launch_delta_apply(s->d, s->ref, static_cast<const double*>(device_buf), w_weight, s->st);
}

int sgdnet_solver_export_delta(sgdnet_solver* s, void* device_buf) {
  int rc = sgdnet_solver_export_delta_async(s, device_buf);
  if (rc) return rc;
  SGD_HIP_TRY(hipStreamSynchronize(s->st));
  return SGDNET_OK;
}

int sgdnet_solver_apply_merged(sgdnet_solver* s, const void* device_buf, double w_weight) {
  int rc = sgdnet_solver_apply_merged_async(s, device_buf, w_weight);
  if (rc) return rc;
  SGD_HIP_TRY(hipStreamSynchronize(s->st));
  return SGDNET_OK;
}

int64_t sgdnet_auto_batch(double max_sample_sqnorm, double max_feature_mean_sq) {
  if (!(max_sample_sqnorm > 0.0) || !(max_feature_mean_sq > 0.0)) return 64;
  const double b = 2.0 * max_sample_sqnorm / max_feature_mean_sq;
  if (!(b < 131072.0)) return 131072;
  return b < 64.0 ? 64 : (int64_t)b;
}

int64_t sgdnet_shard_window(int64_t window, int64_t draws_per_shard) {
  if (window < 1 || draws_per_shard <= window || draws_per_shard % window == 0) return window;
  const int64_t rounds = (draws_per_shard + window - 1) / window;          // >= 2
  const int64_t longer = (draws_per_shard + rounds - 2) / (rounds - 1);
  return longer <= window + window / 8 ? longer : window;
}

}  // extern "C"

// w = g_sum = g_memory = g_sum_intercept = 0, intercept = b0 (K values): the state a fit starts
// from (driver.cpp restarts a lambda from here when the automatic staleness window diverged)
int solver_reset_state(sgdnet_solver* s, const double* b0) {
  SGD_HIP_TRY(hipSetDevice(s->device));
  if (s->m_in_rec) {              // the array is cleared below; the records take it over again at the next batched run
    s->m_in_rec = false;
    s->d.m_rec = 0;
    s->d.m_base = reinterpret_cast<char*>(s->d.M);
    s->d.m_stride = 8;
    drop_graph(s);
  }
  const SagaDev& d = s->d;
  const size_t K = (size_t)d.K;
  SGD_HIP_TRY(hipMemsetAsync(d.w, 0, sizeof(double) * K * (size_t)d.p, s->st));
  SGD_HIP_TRY(hipMemsetAsync(d.G, 0, sizeof(double) * K * (size_t)d.p, s->st));
  SGD_HIP_TRY(hipMemsetAsync(d.M, 0, sizeof(double) * K * (size_t)d.n, s->st));
  SGD_HIP_TRY(hipMemsetAsync(d.gb, 0, sizeof(double) * K, s->st));
  SGD_HIP_TRY(hipMemcpyAsync(d.b, b0, sizeof(double) * K, hipMemcpyHostToDevice, s->st));
  SGD_HIP_TRY(hipMemsetAsync(d.lag, 0, sizeof(unsigned) * (size_t)d.p, s->st));
  SGD_HIP_TRY(hipStreamSynchronize(s->st));
  s->w_prev_valid = false;
  return SGDNET_OK;
}

// Binned form, recovery from a bin overflow (driver.cpp): true when the last synchronisation found one.
bool solver_bin_overflowed(const sgdnet_solver* s) { return s && s->bin_overflowed; }

// After an overflow: twice the room in every bin (rebuilt by the next run); after three doublings the
// solver gives the binned form up -- the atomic form takes over where there is one (n_classes <= 16),
// otherwise SGDNET_EUNSUPPORTED (no batched form left: the caller falls back to the exact iteration).
int solver_grow_bins(sgdnet_solver* s) {
  s->bin_overflowed = false;
  if (s->bin_slack < 64.0) {
    s->bin_slack *= 2.0;
    return SGDNET_OK;
  }
  s->bin_disabled = true;
  if (s->d.K > 16) {
    set_error("batched mode: the binned form keeps overflowing and more than 16 classes have no other batched form");
    return SGDNET_EUNSUPPORTED;
  }
  return SGDNET_OK;
}

// Is there a batched form for this solver at this window?  (More than 16 classes need the binned form,
// which needs feature ranges: at most 2048 of them, sparse x.)
bool solver_batched_available(sgdnet_solver* s, int64_t batch) {
  if (!s) return false;
  if (s->d.K <= 16) return true;
  if (s->d.K > 64) return false;
  if (!s->sparse) return true;                  // dense x: the class-lane form
  if (ensure_binned(s, batch < 1 ? 1 : batch) != SGDNET_OK) return false;
  return s->d.R > 0 && !s->bin_disabled;
}

namespace sgdnet {

int solver_create_adopting(const sgdnet_problem* pb, DeviceSetup& S, sgdnet_solver** out) {
  return solver_create_impl(pb, &S, out);
}

}  // namespace sgdnet
