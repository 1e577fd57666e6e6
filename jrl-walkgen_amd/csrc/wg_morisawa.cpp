// Morisawa-2007 analytic walks, host side of the C ABI (include/wg_mpc.h: wg_morisawa_defaults, _block_bytes, _block_unpack,
// _length, _coshsinh, _system, _solve, _solve_fleet, _resolve, _resolve_fleet, _sample, and the wg_morisawa_long_* forms of all but
// the first and _coshsinh: walks of up to WG_MORISAWA_LONG_MAX_STEPS steps, Z as a band).
//
// The arithmetic is wg_morisawa_math.hpp, the one text this file and the kernels (wg_morisawa_kernels.hpp) compile: a block or a
// sample made here has the bytes the device makes.  Nothing here calls the device, so these run where there is none.
#include <cstring>
#include <vector>

#include "wg_morisawa_math.hpp"

namespace {

// lng: the long family (the band, wg_morisawa_long_*) -- its own cap, layout and solve; everything else is one text for both
bool smax_ok(int smax, bool lng = false) { return smax >= 2 && smax <= (lng ? WG_MORISAWA_LONG_MAX_STEPS : WG_MORISAWA_MAX_STEPS); }
wg::MoLayout layout_of(int smax, bool lng) { return lng ? wg::mo_layout_long(smax) : wg::mo_layout(smax); }

int solve_host(bool lng, const wg_morisawa_model_t *models, bool per_gait, int B, int smax, const wg_rel_step_t *steps,
               const int *n_steps, const double *init_feet, const double *com0, void *blocks, int *status) {
  if (!models || B < 0 || !smax_ok(smax, lng) || !steps || !n_steps || !init_feet || !com0 || !blocks || !status) return WG_ERR_BAD_ARG;
  const wg::MoLayout L = layout_of(smax, lng);
  std::vector<double> W((size_t)L.work_words);
  for (int b = 0; b < B; b++) {
    const wg_morisawa_model_t &m = models[per_gait ? b : 0];
    double *blk = static_cast<double *>(blocks) + (size_t)b * L.words;
    if (lng) {                                                 // the long solve writes the block itself, behind its factor
      status[b] = wg::mo_solve_long(wg::MoHostExec(), m, smax, steps + (size_t)b * smax, n_steps[b], init_feet + 6 * (size_t)b,
                                    com0 + 3 * (size_t)b, W.data(), L, blk, nullptr);
      continue;
    }
    const int rc = wg::mo_solve(wg::MoHostExec(), m, smax, steps + (size_t)b * smax, n_steps[b], init_feet + 6 * (size_t)b,
                                com0 + 3 * (size_t)b, W.data(), L, nullptr);
    status[b] = rc;
    if (rc != WG_OK) continue;
    for (int e = 0; e < L.words; e++) blk[e] = wg::mo_image_word(W.data(), L, e);
  }
  return WG_OK;
}

// the re-plan from kept factors (mo_resolve, mo_resolve_long): gait b's step count is its factor block's
int resolve_host(bool lng, const wg_morisawa_model_t *models, bool per_gait, int B, int smax, const void *factors, int n_factors,
                 const int *factor_of, const wg_rel_step_t *steps, const double *init_feet, const double *com0, void *blocks, int *status) {
  if (!models || B < 0 || !smax_ok(smax, lng) || !factors || n_factors < 1 || !steps || !init_feet || !com0 || !blocks || !status)
    return WG_ERR_BAD_ARG;
  const wg::MoLayout L = layout_of(smax, lng);
  std::vector<double> W((size_t)L.work_words);
  for (int b = 0; b < B; b++) {
    const wg_morisawa_model_t &m = models[per_gait ? b : 0];
    const int f = factor_of ? factor_of[b] : 0;
    if (f < 0 || f >= n_factors) { status[b] = WG_MORISAWA_BAD_INPUT; continue; }
    const double *fac = static_cast<const double *>(factors) + (size_t)f * L.words;
    double *blk = static_cast<double *>(blocks) + (size_t)b * L.words;
    if (lng) {
      status[b] = wg::mo_resolve_long(wg::MoHostExec(), m, smax, fac, steps + (size_t)b * smax, init_feet + 6 * (size_t)b,
                                      com0 + 3 * (size_t)b, W.data(), L, blk);
      continue;
    }
    const int rc = wg::mo_resolve(wg::MoHostExec(), m, smax, fac, steps + (size_t)b * smax, init_feet + 6 * (size_t)b,
                                  com0 + 3 * (size_t)b, W.data(), L);
    status[b] = rc;
    if (rc != WG_OK) continue;
    for (int e = 0; e < L.words; e++) blk[e] = wg::mo_image_word(W.data(), L, e);
  }
  return WG_OK;
}

int unpack_host(bool lng, const void *block, int smax, wg_morisawa_view_t *v) {
  if (!block || !v || !smax_ok(smax, lng)) return WG_ERR_BAD_ARG;
  const double *b = static_cast<const double *>(block);
  if (!(lng ? wg::mo_block_ok_long(b, smax) : wg::mo_block_ok(b, smax))) return WG_MORISAWA_BAD_INPUT;
  const wg::MoLayout L = layout_of(smax, lng);
  const int *hdr = reinterpret_cast<const int *>(b);
  memset(v, 0, sizeof *v);
  v->n_steps = hdr[0]; v->n_int = hdr[1]; v->n = hdr[2]; v->smax = hdr[3];
  v->com_height = b[2]; v->t_total = b[3];
  v->dT = b + L.o_dT; v->omega = b + L.o_om; v->tref = b + L.o_tref;
  v->zmp_x = b + L.o_zx; v->cog_x = b + L.o_cx; v->zmp_y = b + L.o_zy; v->cog_y = b + L.o_cy;
  v->Vx = b + L.o_vx; v->Wx = b + L.o_wx; v->Vy = b + L.o_vy; v->Wy = b + L.o_wy;
  v->left = b + L.o_left; v->right = b + L.o_right;
  v->left_type = reinterpret_cast<const int *>(b + L.o_nat); v->right_type = v->left_type + L.imax;
  v->profile_x = b + L.o_zpx; v->profile_y = b + L.o_zpy;
  v->support = b + L.o_sup;
  v->wx = b + L.o_rhs; v->wy = v->wx + L.nmax; v->yx = v->wy + L.nmax; v->yy = v->yx + L.nmax;
  v->piv = reinterpret_cast<const int *>(b + L.o_piv);
  v->lu = b + L.o_lu; v->lu_pitch = lng ? wg::kMoBand : L.nmax;
  return WG_OK;
}

int sample_host(bool lng, int B, int smax, const void *blocks, const int *status, double t_start, double T, int lcap, double *zmp_x_tm,
                double *zmp_y_tm, double *com_tm, double *left_tm, int *left_type_tm, double *right_tm, int *right_type_tm, int *length) {
  if (!blocks || B < 0 || !smax_ok(smax, lng) || lcap < 1 || !wg::mo_finite(T) || !(T > 0.0) || !wg::mo_finite(t_start) || t_start < 0.0)
    return WG_ERR_BAD_ARG;
  const wg::MoLayout L = layout_of(smax, lng);
  std::vector<double> clock((size_t)lcap + 1);
  double t = t_start;
  for (int k = 0; k <= lcap; k++) { clock[k] = t; t += T; }
  const size_t Bs = (size_t)B;
  for (int b = 0; b < B; b++) {
    const double *blk = static_cast<const double *>(blocks) + (size_t)b * L.words;
    int len = status ? status[b] : WG_OK;
    if (len >= 0)
      len = (lng ? wg::mo_block_ok_long(blk, smax) : wg::mo_block_ok(blk, smax)) ? wg::mo_count(clock.data(), lcap, blk[3]) : WG_MORISAWA_BAD_INPUT;
    if (len > lcap) len = WG_MORISAWA_CAPACITY;
    if (length) length[b] = len;
    if (len <= 0) continue;
    for (int k = 0; k < lcap; k++) {
      wg::MoSample o;
      wg::mo_sample(blk, L, clock[k < len ? k : len - 1], o);
      const size_t r = (size_t)k;
      if (zmp_x_tm) zmp_x_tm[r * Bs + b] = o.zx;
      if (zmp_y_tm) zmp_y_tm[r * Bs + b] = o.zy;
      if (com_tm)
        for (int c = 0; c < 4; c++) com_tm[(r * 4 + c) * Bs + b] = o.com[c];
      if (left_tm)
        for (int c = 0; c < 6; c++) left_tm[(r * 6 + c) * Bs + b] = o.left[c];
      if (right_tm)
        for (int c = 0; c < 6; c++) right_tm[(r * 6 + c) * Bs + b] = o.right[c];
      if (left_type_tm) left_type_tm[r * Bs + b] = o.ltype;
      if (right_type_tm) right_type_tm[r * Bs + b] = o.rtype;
    }
  }
  return WG_OK;
}

}  // namespace

extern "C" {

void wg_morisawa_defaults(wg_morisawa_model_t *m) {
  if (!m) return;
  memset(m, 0, sizeof *m);
  m->T = 0.005;
  m->t_single = 0.78;
  m->t_double = 0.02;
  m->step_height = 0.07;
  m->omega = 0.0;
}

size_t wg_morisawa_block_bytes(int smax) { return smax_ok(smax) ? (size_t)wg::mo_layout(smax).words * sizeof(double) : 0; }

int wg_morisawa_block_unpack(const void *block, int smax, wg_morisawa_view_t *v) { return unpack_host(false, block, smax, v); }

int wg_morisawa_length(const wg_morisawa_model_t *model, int n_steps, double t_start) {
  if (!model) return WG_MORISAWA_BAD_INPUT;
  return wg::mo_length(*model, n_steps, t_start);
}

int wg_morisawa_coshsinh(double x, double *cosh_x, double *sinh_x) {
  if (!cosh_x || !sinh_x) return WG_ERR_BAD_ARG;
  if (!(x >= 0.0 && x <= wg::kMoArgMax)) return WG_MORISAWA_BAD_INPUT;
  wg::mo_coshsinh(x, *cosh_x, *sinh_x);
  return WG_OK;
}

int wg_morisawa_system(const wg_morisawa_model_t *model, int n_steps, const wg_rel_step_t *steps, const double *init_feet,
                       const double *com0, double *Z, double *wx, double *wy) {
  if (!model || !steps || !init_feet || !com0 || !Z || !wx || !wy) return WG_ERR_BAD_ARG;
  if (n_steps < 2 || n_steps > WG_MORISAWA_MAX_STEPS) return WG_MORISAWA_BAD_INPUT;
  const wg::MoLayout L = wg::mo_layout(n_steps);
  std::vector<double> W((size_t)L.work_words);
  const int rc = wg::mo_solve(wg::MoHostExec(), *model, n_steps, steps, n_steps, init_feet, com0, W.data(), L, Z);
  if (rc != WG_OK && rc != WG_MORISAWA_SINGULAR) return rc;
  const int n = 4 * n_steps + 8;
  for (int e = 0; e < n; e++) { wx[e] = W[L.o_rhs + e]; wy[e] = W[L.o_rhs + L.nmax + e]; }
  return n;
}

int wg_morisawa_solve(const wg_morisawa_model_t *model, int B, int smax, const wg_rel_step_t *steps, const int *n_steps,
                      const double *init_feet, const double *com0, void *blocks, int *status) {
  return solve_host(false, model, false, B, smax, steps, n_steps, init_feet, com0, blocks, status);
}

int wg_morisawa_solve_fleet(const wg_morisawa_model_t *models, int B, int smax, const wg_rel_step_t *steps, const int *n_steps,
                            const double *init_feet, const double *com0, void *blocks, int *status) {
  return solve_host(false, models, true, B, smax, steps, n_steps, init_feet, com0, blocks, status);
}

int wg_morisawa_resolve(const wg_morisawa_model_t *model, int B, int smax, const void *factors, int n_factors, const int *factor_of,
                        const wg_rel_step_t *steps, const double *init_feet, const double *com0, void *blocks, int *status) {
  return resolve_host(false, model, false, B, smax, factors, n_factors, factor_of, steps, init_feet, com0, blocks, status);
}

int wg_morisawa_resolve_fleet(const wg_morisawa_model_t *models, int B, int smax, const void *factors, int n_factors,
                              const int *factor_of, const wg_rel_step_t *steps, const double *init_feet, const double *com0,
                              void *blocks, int *status) {
  return resolve_host(false, models, true, B, smax, factors, n_factors, factor_of, steps, init_feet, com0, blocks, status);
}

int wg_morisawa_sample(int B, int smax, const void *blocks, const int *status, double t_start, double T, int lcap, double *zmp_x_tm,
                       double *zmp_y_tm, double *com_tm, double *left_tm, int *left_type_tm, double *right_tm, int *right_type_tm,
                       int *length) {
  return sample_host(false, B, smax, blocks, status, t_start, T, lcap, zmp_x_tm, zmp_y_tm, com_tm, left_tm, left_type_tm, right_tm,
                     right_type_tm, length);
}

// ---- the long family: the same calls with the band behind them ----
size_t wg_morisawa_long_block_bytes(int smax) { return smax_ok(smax, true) ? (size_t)wg::mo_layout_long(smax).words * sizeof(double) : 0; }

int wg_morisawa_long_block_unpack(const void *block, int smax, wg_morisawa_view_t *v) { return unpack_host(true, block, smax, v); }

int wg_morisawa_long_length(const wg_morisawa_model_t *model, int n_steps, double t_start) {
  if (!model) return WG_MORISAWA_BAD_INPUT;
  return wg::mo_length(*model, n_steps, t_start, WG_MORISAWA_LONG_MAX_STEPS);
}

int wg_morisawa_long_system(const wg_morisawa_model_t *model, int n_steps, const wg_rel_step_t *steps, const double *init_feet,
                            const double *com0, double *Zband, double *wx, double *wy) {
  if (!model || !steps || !init_feet || !com0 || !Zband || !wx || !wy) return WG_ERR_BAD_ARG;
  if (!smax_ok(n_steps, true)) return WG_MORISAWA_BAD_INPUT;
  const wg::MoLayout L = wg::mo_layout_long(n_steps), Lw = wg::mo_work_long(L);
  std::vector<double> W((size_t)L.work_words), blk((size_t)L.words);
  const int rc = wg::mo_solve_long(wg::MoHostExec(), *model, n_steps, steps, n_steps, init_feet, com0, W.data(), L, blk.data(), Zband);
  if (rc != WG_OK && rc != WG_MORISAWA_SINGULAR) return rc;
  const int n = 4 * n_steps + 8;
  for (int e = 0; e < n; e++) { wx[e] = W[Lw.o_rhs + e]; wy[e] = W[Lw.o_rhs + L.nmax + e]; }
  return n;
}

int wg_morisawa_long_solve(const wg_morisawa_model_t *model, int B, int smax, const wg_rel_step_t *steps, const int *n_steps,
                           const double *init_feet, const double *com0, void *blocks, int *status) {
  return solve_host(true, model, false, B, smax, steps, n_steps, init_feet, com0, blocks, status);
}

int wg_morisawa_long_solve_fleet(const wg_morisawa_model_t *models, int B, int smax, const wg_rel_step_t *steps, const int *n_steps,
                                 const double *init_feet, const double *com0, void *blocks, int *status) {
  return solve_host(true, models, true, B, smax, steps, n_steps, init_feet, com0, blocks, status);
}

int wg_morisawa_long_resolve(const wg_morisawa_model_t *model, int B, int smax, const void *factors, int n_factors,
                             const int *factor_of, const wg_rel_step_t *steps, const double *init_feet, const double *com0,
                             void *blocks, int *status) {
  return resolve_host(true, model, false, B, smax, factors, n_factors, factor_of, steps, init_feet, com0, blocks, status);
}

int wg_morisawa_long_resolve_fleet(const wg_morisawa_model_t *models, int B, int smax, const void *factors, int n_factors,
                                   const int *factor_of, const wg_rel_step_t *steps, const double *init_feet, const double *com0,
                                   void *blocks, int *status) {
  return resolve_host(true, models, true, B, smax, factors, n_factors, factor_of, steps, init_feet, com0, blocks, status);
}

int wg_morisawa_long_sample(int B, int smax, const void *blocks, const int *status, double t_start, double T, int lcap, double *zmp_x_tm,
                            double *zmp_y_tm, double *com_tm, double *left_tm, int *left_type_tm, double *right_tm,
                            int *right_type_tm, int *length) {
  return sample_host(true, B, smax, blocks, status, t_start, T, lcap, zmp_x_tm, zmp_y_tm, com_tm, left_tm, left_type_tm, right_tm,
                     right_type_tm, length);
}

}  // extern "C"
