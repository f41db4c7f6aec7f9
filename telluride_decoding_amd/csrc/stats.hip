// The statistics object (stats_common.h): its life cycle, the pending reset, the room for its boundary
// windows, and its layout as the solvers see it.
#include "stats_common.h"

int ensure_window_capacity(td_handle* h, td_stats* s, int64_t need) {
  if (need <= s->cap_files) return TD_OK;
  int64_t cap = s->cap_files ? s->cap_files : 64;
  while (cap < need) cap *= 2;
  const size_t per1 = (size_t)stats_window_floats(s, s->c1) * sizeof(float);
  const size_t per2 = (size_t)stats_window_floats(s, s->c2) * sizeof(float);
  void* n1 = nullptr;
  void* n2 = nullptr;
  TD_TRY(td_alloc_async(h, per1 * cap, &n1));
  if (s->c2) TD_TRY(td_alloc_async(h, per2 * cap, &n2));
  if (s->n_files) {
    // (the old windows may have been written from another handle's stream)
    TD_TRY(td_order_after_others(h));
    TD_HIP(h, hipMemcpyAsync(n1, s->win1, per1 * s->n_files, hipMemcpyDeviceToDevice, h->stream));
    if (s->c2)
      TD_HIP(h, hipMemcpyAsync(n2, s->win2, per2 * s->n_files, hipMemcpyDeviceToDevice, h->stream));
  }
  TD_TRY(td_free_async(h, s->win1));
  TD_TRY(td_free_async(h, s->win2));
  s->win1 = reinterpret_cast<float*>(n1);
  s->win2 = reinterpret_cast<float*>(n2);
  s->cap_files = cap;
  return TD_OK;
}

int stats_materialize(td_handle* h, td_stats* s) {
  TD_TRY(td_stats_settle(h, s));
  if (s->fresh_main) {
    TD_HIP(h, hipMemsetAsync(s->g, 0, sizeof(double) * s->off_gxo, h->stream));
    TD_HIP(h, hipMemsetAsync(s->g + s->off_n, 0, sizeof(double) * (s->g_len - s->off_n), h->stream));
    s->fresh_main = false;
  }
  if (s->fresh_tgt) {
    TD_HIP(h, hipMemsetAsync(s->g + s->off_gxo, 0, sizeof(double) * (s->off_n - s->off_gxo), h->stream));
    s->fresh_tgt = false;
  }
  return TD_OK;
}

// Used by solve.hip and loso.hip.
int td_stats_layout(const td_stats* s, int* k1, int* d, int64_t* frames) {
  *k1 = s->k1;
  *d = s->d;
  *frames = s->frames;
  return TD_OK;
}

int td_stats_compact(const td_stats* s, StatsCompact* out) {
  out->ok = s->c2 == 0 && s->d >= 1 && s->pre1 == 0 && s->whole_files && s->frames > 0 && !s->fresh_main &&
            !s->fresh_tgt;
  out->fxx = s->g + s->off_fxx; out->gxo = s->g + s->off_gxo; out->sy = s->g + s->off_sy;
  out->win = s->win1;
  out->c = s->c1; out->l = s->l1; out->d = s->d; out->hw = s->hw;
  out->n_files = s->n_files; out->frames = s->frames;
  return TD_OK;
}

// Used by eig.hip.
// Two views without context (one lag each): the compact sums ARE the dense moments -- sum x x^T [c1][c1],
// sum x2 x2^T [c2][c2], sum x x2^T [c1][c2] and the two column sums -- so td_cca_solve's one-launch dense stage
// reads them where they lie (td_stats_moments would copy them with three launches and two copies).
// *ok = 0: statistics with context (or no second view).
int td_stats_cca_direct(td_handle* h, td_stats* s, const double** xx, const double** yy, const double** xy,
                        const double** sum1, const double** sum2, int* ok) {
  *ok = 0;
  if (!s->c2 || s->l1 != 1 || s->l2 != 1) return TD_OK;
  TD_TRY(stats_materialize(h, s));
  *xx = s->g + s->off_fxx; *yy = s->g + s->off_fyy; *xy = s->g + s->off_gxy;
  *sum1 = s->g + s->off_gxo; *sum2 = s->g + s->off_gyo;
  *ok = 1;
  return TD_OK;
}

int td_stats_dims(const td_stats* s, int* k1, int* k2, int64_t* frames) {
  *k1 = s->k1;
  *k2 = s->k2;
  *frames = s->frames;
  return TD_OK;
}

extern "C" {

int td_stats_create(td_handle* h, int c1, int pre1, int post1, int c2, int pre2, int post2,
                    int d, td_stats** out) {
  if (!h || !out) return td_fail(h, TD_ERR_INVALID, "td_stats_create: NULL argument");
  *out = nullptr;
  TD_REQUIRE(h, c1 > 0, "input_1 must have at least one channel, not %d", c1);
  TD_REQUIRE(h, pre1 >= 0 && post1 >= 0 && pre2 >= 0 && post2 >= 0,
             "context (pre/post) must be >= 0");
  TD_REQUIRE(h, c2 >= 0 && d >= 0, "negative width");
  td_stats* s = new td_stats();
  s->c1 = c1; s->pre1 = pre1; s->post1 = post1;
  s->c2 = c2; s->pre2 = c2 ? pre2 : 0; s->post2 = c2 ? post2 : 0; s->d = d;
  s->l1 = pre1 + 1 + post1;
  s->l2 = c2 ? s->pre2 + 1 + s->post2 : 0;
  s->k1 = s->l1 * c1;
  s->k2 = s->l2 * c2;
  s->hw = s->pre1 + s->post1 + s->pre2 + s->post2 + 1;
  int64_t o = 0;
  s->off_fxx = o; o += (int64_t)s->l1 * c1 * c1;
  s->off_gxo = o; o += (int64_t)s->l1 * (d + 1) * c1;
  s->off_sy = o;  o += d;
  s->off_n = o;   o += 1;
  s->off_fyy = o; o += (int64_t)s->l2 * c2 * c2;
  s->off_gxy = o; o += c2 ? (int64_t)(s->l1 + s->l2 - 1) * c1 * c2 : 0;
  s->off_gyo = o; o += (int64_t)s->l2 * c2;
  s->g_len = o;
  void* g = nullptr;
  const int rc = td_alloc_async(h, sizeof(double) * s->g_len, &g);
  if (rc != TD_OK) {
    delete s;
    return rc;
  }
  s->g = reinterpret_cast<double*>(g);
  TD_HIP(h, hipMemsetAsync(s->g, 0, sizeof(double) * s->g_len, h->stream));
  *out = s;
  return TD_OK;
}

int td_stats_destroy(td_handle* h, td_stats* s) {
  if (!s) return TD_OK;
  if (s->dscratch || s->djobs || s->dscale) {
    // (blocks of a deferred finalize: kernels of other streams may still read them)
    hipDeviceSynchronize();
    if (s->dscratch) hipFree(s->dscratch);
    if (s->djobs) hipFree(s->djobs);
    if (s->dscale) hipFree(s->dscale);
  }
  if (h) {
    // stream-ordered: after everything queued so far on this and the other handles' streams;
    // nothing waits (td_free_async)
    td_free_async(h, s->g);
    td_free_async(h, s->win1);
    td_free_async(h, s->win2);
    td_free_async(h, s->chan_tab);
  } else {
    hipDeviceSynchronize();
    if (s->g) hipFree(s->g);
    if (s->win1) hipFree(s->win1);
    if (s->win2) hipFree(s->win2);
    if (s->chan_tab) hipFree(s->chan_tab);
  }
  delete s;
  return TD_OK;
}

int td_stats_reset(td_handle* h, td_stats* s) {
  if (!h || !s) return td_fail(h, TD_ERR_INVALID, "td_stats_reset: NULL argument");
  if (stats_fusable(s) || stats_one_pass(s)) {
    // nothing is queued: the next accumulate call overwrites (td_stats::fresh_*)
    s->fresh_main = s->fresh_tgt = true;
  } else {
    TD_HIP(h, hipMemsetAsync(s->g, 0, sizeof(double) * s->g_len, h->stream));
  }
  s->n_files = 0;
  s->frames = 0;
  s->tab_ready = false;
  s->whole_files = true;
  s->pending = false;            // (a finalize nobody asked for: its sums are being discarded)
  return TD_OK;
}

int td_stats_counts(td_handle* h, const td_stats* s, int64_t* frames, int64_t* files) {
  if (!s) return td_fail(h, TD_ERR_INVALID, "td_stats_counts: NULL statistics");
  if (frames) *frames = s->frames;
  if (files) *files = s->n_files;
  return TD_OK;
}

}  // extern "C"
