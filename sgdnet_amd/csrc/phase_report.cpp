// What the kernels' phase stamps (SagaDev::dbg) say, printed after an exact launch (sgdnet_solver_run) and after a
// profiled batched epoch (sgdnet_solver_profile_epoch).  Development builds only, EXTRA_FLAGS=-DSGDNET_PHASE_TIMING:
// without the define this file is empty.  The text is read by eye against the logs under profiles/.
#ifdef SGDNET_PHASE_TIMING
#include <stdio.h>
#include <stdlib.h>

#include <algorithm>
#include <vector>

#include "solver_state.hpp"

namespace sgdnet {

int phase_report_exact(const sgdnet_solver* s, const ExactPlan& plan, int epochs, int64_t draws_per_epoch) {
  if (plan.form == ExactForm::kDenseSmall2 && s->d.dbg && epochs > 0) {
    unsigned long long c[5];
    SGD_HIP_TRY(hipMemcpy(c, s->d.dbg + 24, sizeof(c), hipMemcpyDeviceToHost));
    (void)hipMemset(s->d.dbg + 24, 0, sizeof(c));
    const double its = (double)epochs * (double)draws_per_epoch;
    fprintf(stderr, "[sgdnet] small dense kernel with feeder, consumer cycles per draw: slot+history %.0f, dot %.0f, gradient+store %.0f, "
                    "intercept %.0f, step+penalty+average %.0f\n", c[0] / its, c[1] / its, c[2] / its, c[3] / its, c[4] / its);
  }
  if (plan.form == ExactForm::kSparseK1m && s->d.dbg && epochs > 0) {
    (void)hipDeviceSynchronize();
    unsigned long long c[5];
    SGD_HIP_TRY(hipMemcpy(c, s->d.dbg + 16, sizeof(c), hipMemcpyDeviceToHost));
    (void)hipMemset(s->d.dbg + 16, 0, sizeof(c));
    const double its = (double)epochs * (double)draws_per_epoch;
    fprintf(stderr, "[sgdnet] multi-consumer sparse kernel, polls per draw: slot %.2f, registration %.2f, dependency %.2f, chain %.2f, barrier %.3f\n",
            c[0] / its, c[1] / its, c[2] / its, c[3] / its, c[4] / its);
  } else if (plan.form == ExactForm::kSparseK1x && s->d.dbg && epochs > 0) {
    (void)hipDeviceSynchronize();
    unsigned long long c[12];
    SGD_HIP_TRY(hipMemcpy(c, s->d.dbg, sizeof(c), hipMemcpyDeviceToHost));
    (void)hipMemset(s->d.dbg, 0, sizeof(c));
    fprintf(stderr, "[sgdnet] producer/consumer sparse kernel, %d x %lld draws: producer waited %llu times (%llu polls), consumer %llu times (%llu polls)\n",
            epochs, (long long)draws_per_epoch, c[9], c[8], c[11], c[10]);
    const double its = (double)epochs * (double)draws_per_epoch;
    fprintf(stderr, "[sgdnet]   consumer cycles per draw: slot+requests %.0f, catch-up+sum %.0f, gradient %.0f, scale+intercept+early threshold %.0f, "
                    "step+stores %.0f, forward %.0f\n", c[0] / its, c[1] / its, c[2] / its, c[3] / its, c[4] / its, c[5] / its);
  }
  if (plan.form == ExactForm::kDenseWide && s->d.dbg && epochs > 0) {   // development aid: shader-clock cycles of thread 0 per phase of the wide kernel
    unsigned long long ph[6];
    SGD_HIP_TRY(hipMemcpy(ph, s->d.dbg, sizeof(ph), hipMemcpyDeviceToHost));
    (void)hipMemset(s->d.dbg, 0, sizeof(ph));
    const double its = (double)epochs * (double)draws_per_epoch;
    fprintf(stderr, "[sgdnet] wide exact kernel, cycles per iteration (thread 0): loads+dot+sum %.0f, scale %.0f, barrier A %.0f, "
                    "class %.0f, barrier B %.0f, step %.0f\n",
            (double)ph[0] / its, (double)ph[1] / its, (double)ph[2] / its, (double)ph[3] / its, (double)ph[4] / its, (double)ph[5] / its);
  }
  return SGDNET_OK;
}

int phase_report_batched(const sgdnet_solver* s, int64_t batch, bool fused_prof) {
  if (s->d.dbg && fused_prof) {   // fused epoch kernel: thread 0's time per phase, summed over the rounds
    const int grid = s->d.V * s->d.v_bps;
    std::vector<unsigned long long> t(16 * 1024);
    SGD_HIP_TRY(hipMemcpy(t.data(), s->d.dbg, sizeof(unsigned long long) * t.size(), hipMemcpyDeviceToHost));
    static const char* nm[8] = {"stage w + ids", "draw loop", "publish slab", "wait shard (1)", "slice sweep", "merge",
                                "store + arrive", "wait shard (2)"};
    unsigned long long first = ~0ull, last = 0;
    for (int b = 0; b < grid; ++b) {
      first = std::min(first, t[b * 16 + 14]);
      last = std::max(last, t[b * 16 + 15]);
    }
    fprintf(stderr, "[phase] fused epoch kernel: span seen by the workgroups %.1f us (%d workgroups)\n", (double)(last - first) / 100.0, grid);
    double tot_mean = 0;
    for (int ph = 0; ph < 8; ++ph) {
      double sum = 0, mx = 0, mn = 1e30;
      for (int b = 0; b < grid; ++b) {
        const double dt = (double)t[b * 16 + ph] / 100.0;
        sum += dt; mx = std::max(mx, dt); mn = std::min(mn, dt);
      }
      tot_mean += sum / grid;
      fprintf(stderr, "[phase] %-16s per epoch: mean %7.1f us  min %7.1f  max %7.1f\n", nm[ph], sum / grid, mn, mx);
    }
    fprintf(stderr, "[phase] sum of the means %.1f us\n", tot_mean);
    // the epoch's boundary, once per launch: slots 10 / 8 / 9
    static const char* bn[3] = {"entry -> go seen", "go -> draw loop 0", "last stores -> out"};
    const int bs[3] = {10, 8, 9};
    for (int k = 0; k < 3; ++k) {
      double sum = 0, mx = 0, mn = 1e30;
      for (int b = 0; b < grid; ++b) {
        const double dt = (double)t[b * 16 + bs[k]] / 100.0;
        sum += dt; mx = std::max(mx, dt); mn = std::min(mn, dt);
      }
      fprintf(stderr, "[phase] %-18s per launch: mean %6.1f us  min %6.1f  max %6.1f\n", bn[k], sum / grid, mn, mx);
    }
    for (int v = 0; v < s->d.V; ++v) {
      double a0 = 0, a1 = 0;
      for (int b = v * s->d.v_bps; b < (v + 1) * s->d.v_bps; ++b) {
        a0 += (double)(t[b * 16 + 14] - first) / 100.0;
        a1 += (double)(t[b * 16 + 15] - first) / 100.0;
      }
      fprintf(stderr, "[phase]   shard %d: mean start %.1f us, mean end %.1f us\n", v, a0 / s->d.v_bps, a1 / s->d.v_bps);
    }
  } else
  if (s->d.dbg && plan(s, batch, batch).form == BatchForm::kBinned) {   // binned form: slots 0-5 gather, 6-10 range sweep
    std::vector<unsigned long long> t(16 * 1024);
    SGD_HIP_TRY(hipMemcpy(t.data(), s->d.dbg, sizeof(unsigned long long) * t.size(), hipMemcpyDeviceToHost));
    static const char* nm[10] = {"gather: init", "gather: draw loop", "gather: barrier", "gather: reserve runs",
                                 "gather: place entries", "", "sweep: zero + first entries", "sweep: entries -> LDS",
                                 "sweep: barrier", "sweep: update features"};
    for (int ph = 0; ph < 10; ++ph) {
      if (ph == 5) continue;
      double sum = 0, mx = 0;
      int cnt = 0;
      for (int b = 0; b < 1024; ++b) {
        if (!t[b * 16 + ph] || !t[b * 16 + ph + 1] || t[b * 16 + ph + 1] < t[b * 16 + ph]) continue;
        const double dt = (double)(t[b * 16 + ph + 1] - t[b * 16 + ph]) / 100.0;
        sum += dt; mx = std::max(mx, dt); ++cnt;
      }
      if (cnt) fprintf(stderr, "[phase] %-28s mean %6.2f us max %6.2f us (%d workgroups)\n", nm[ph], sum / cnt, mx, cnt);
    }
    for (int k0 : {0, 6}) {
      unsigned long long first = ~0ull, last = 0;
      const int k1 = k0 == 0 ? 5 : 10;
      for (int b = 0; b < 1024; ++b) {
        if (t[b * 16 + k0] && t[b * 16 + k0] < first) first = t[b * 16 + k0];
        if (t[b * 16 + k1] > last) last = t[b * 16 + k1];
      }
      fprintf(stderr, "[phase] %s span seen by the workgroups %.2f us\n", k0 == 0 ? "gather" : "sweep", (double)(last - first) / 100.0);
      std::vector<double> st, en;
      for (int b = 0; b < 1024; ++b)
        if (t[b * 16 + k0] && t[b * 16 + k1] >= t[b * 16 + k0]) {
          st.push_back((double)(t[b * 16 + k0] - first) / 100.0);
          en.push_back((double)(t[b * 16 + k1] - first) / 100.0);
        }
      std::sort(st.begin(), st.end());
      std::sort(en.begin(), en.end());
      if (!st.empty())
        fprintf(stderr, "[phase]   workgroup start offsets: p10 %.1f p50 %.1f p90 %.1f max %.1f us; end offsets: p10 %.1f p50 %.1f p90 %.1f max %.1f us\n",
                st[st.size() / 10], st[st.size() / 2], st[st.size() * 9 / 10], st.back(), en[en.size() / 10], en[en.size() / 2],
                en[en.size() * 9 / 10], en.back());
    }
  } else
  if (s->d.dbg) {   // stamps of the epoch's last gather launch (the tail batch unless batch divides the epoch)
    std::vector<unsigned long long> t(16 * 256);
    SGD_HIP_TRY(hipMemcpy(t.data(), s->d.dbg, sizeof(unsigned long long) * t.size(), hipMemcpyDeviceToHost));
    unsigned long long first = ~0ull, last = 0;
    for (int b = 0; b < 256; ++b) {
      if (t[b * 16] && t[b * 16] < first) first = t[b * 16];
      if (t[b * 16 + 5] > last) last = t[b * 16 + 5];
    }
    if (getenv("SGDNET_PHASE_DUMP")) {
      fprintf(stderr, "[phase-dump] draw loop us by workgroup:");
      for (int b = 0; b < 256; ++b) fprintf(stderr, " %.1f", (double)(t[b * 16 + 2] - t[b * 16 + 1]) / 100.0);
      fprintf(stderr, "\n[phase-dump] draw loop + barrier us by workgroup:");
      for (int b = 0; b < 256; ++b) fprintf(stderr, " %.1f", (double)(t[b * 16 + 3] - t[b * 16 + 1]) / 100.0);
      fprintf(stderr, "\n[phase-dump] start offset us by workgroup:");
      for (int b = 0; b < 256; ++b) fprintf(stderr, " %.1f", (double)(t[b * 16 + 1] - first) / 100.0);
      fprintf(stderr, "\n");
    }
    static const char* nm[11] = {"lds zero+sync", "draw loop", "barrier", "slab flush", "d0 partial", "",
                                 "stream idx", "record loads", "w gather", "M exchange", "scatter"};
    fprintf(stderr, "[phase] kernel span %.2f us (memtime ticks at 100 MHz)\n", (double)(last - first) / 100.0);
    double start_spread = 0;
    for (int b = 0; b < 256; ++b) if (t[b * 16]) start_spread = std::max(start_spread, (double)(t[b * 16] - first));
    fprintf(stderr, "[phase] workgroup start spread %.2f us\n", start_spread / 100.0);
    for (int ph = 0; ph < 11; ++ph) {
      if (ph == 5) continue;
      const int a = ph < 5 ? ph : ph, bslot = a + 1;
      double sum = 0, mx = 0; int cnt = 0;
      for (int b = 0; b < 256; ++b) {
        if (!t[b * 16 + a] || !t[b * 16 + bslot]) continue;
        const double dt = (double)(t[b * 16 + bslot] - t[b * 16 + a]) / 100.0;
        sum += dt; mx = std::max(mx, dt); ++cnt;
      }
      if (cnt) fprintf(stderr, "[phase] %-14s mean %6.2f us max %6.2f us\n", nm[ph], sum / cnt, mx);
    }
  }
  return SGDNET_OK;
}

}  // namespace sgdnet
#endif
