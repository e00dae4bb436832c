// api_ccs.hip -- the CCS matrices behind include/lf.h: their upload and structure
// (lf_ccs_*), the sparse Mz products (lf_dev_mz_*) and the relation checks.
#include <algorithm>
#include <cstdlib>
#include <memory>

#include "api_internal.hpp"

extern "C" {

// ---------------------------------------------------------------- sparse Mz products
void lf_ccs_destroy(lf_ccs *M) { delete M; }

int lf_ccs_shape(const lf_ccs *M, int *t, size_t *m, size_t *n, size_t *l, int *q, int *degree) {
  if (!M) return LF_ERR_INVALID_ARG;
  if (t) *t = M->dev.t;
  if (m) *m = M->dev.m;
  if (n) *n = M->dev.n;
  if (l) *l = M->l;
  if (q) *q = M->structured ? (int)M->S_off.size() - 1 : 0;
  if (degree) *degree = M->degree;
  return M->structured ? LF_OK : LF_ERR_INVALID_ARG;
}

int lf_ccs_get_structure(const lf_ccs *M, uint64_t *cc, int *S_off, int *S_idx) {
  if (!M || !M->structured) return LF_ERR_INVALID_ARG;
  if (cc) std::copy(M->c.begin(), M->c.end(), cc);
  if (S_off) std::copy(M->S_off.begin(), M->S_off.end(), S_off);
  if (S_idx) std::copy(M->S_idx.begin(), M->S_idx.end(), S_idx);
  return LF_OK;
}

const uint64_t *lf_ccs_c_device(const lf_ccs *M) { return M ? M->c_dev : nullptr; }

int lf_ccs_is_scalar(const lf_ccs *M) { return M && M->dev.sval ? 1 : 0; }

int lf_ccs_is_reordered(const lf_ccs *M) { return M && M->dev.vh && M->dev.vc ? 1 : 0; }

int lf_ccs_row_live(const lf_ccs *M, int j, uint8_t *out) {
  if (!M || !out || j < 0 || j >= M->dev.t) return LF_ERR_INVALID_ARG;
  std::copy(M->live.begin() + (size_t)j * M->dev.m, M->live.begin() + (size_t)(j + 1) * M->dev.m, out);
  return LF_OK;
}

int lf_ccs_set_structure(lf_ctx *c, lf_ccs *M, size_t l, int degree, int q, const uint64_t *cc, const int *S_off,
                         const int *S_idx, int repr) {
  if (!c || !M || q < 1 || !cc || !S_off || !S_idx || degree < 1) return LF_ERR_INVALID_ARG;
  DevGuard g(c);
  LF_TRY(check_repr(c, repr));
  const int d = M->dev.d;
  if (l + 1 > M->dev.n) return fail(c, LF_ERR_INVALID_ARG, "CCS: l + 1 > n");
  if (S_off[0] != 0) return fail(c, LF_ERR_INVALID_ARG, "CCS: S_off[0] must be 0");
  for (int i = 0; i < q; i++) {
    if (S_off[i + 1] < S_off[i]) return fail(c, LF_ERR_INVALID_ARG, "CCS: S_off must not decrease");
    if (S_off[i + 1] - S_off[i] > degree) return fail(c, LF_ERR_INVALID_ARG, "CCS: a multiset exceeds the degree");
  }
  for (int k = 0; k < S_off[q]; k++)
    if (S_idx[k] < 0 || S_idx[k] >= M->dev.t) return fail(c, LF_ERR_INVALID_ARG, "CCS: multiset index out of range");
  M->c.assign(cc, cc + (size_t)q * d);
  if (repr == LF_REPR_MONTGOMERY)
    for (auto &x : M->c) x = gl::from_mont(x);
  M->S_off.assign(S_off, S_off + q + 1);
  M->S_idx.assign(S_idx, S_idx + S_off[q]);
  M->l = l;
  M->degree = degree;
  if (!M->c_dev || M->c_dev_elems < (size_t)q * d) {
    void *p = nullptr;
    LF_HIP(c, hipMalloc(&p, (size_t)q * d * 8));
    M->bufs.push_back(p);
    M->c_dev = (uint64_t *)p;
    M->c_dev_elems = (size_t)q * d;
  }
  LF_HIP(c, hipMemcpyAsync(M->c_dev, M->c.data(), (size_t)q * d * 8, hipMemcpyHostToDevice, c->cur));
  const size_t s_elems = (size_t)q + 1 + M->S_idx.size();
  if (!M->S_dev || M->S_dev_elems < s_elems) {
    void *p = nullptr;
    LF_HIP(c, hipMalloc(&p, s_elems * sizeof(int)));
    M->bufs.push_back(p);
    M->S_dev = (int *)p;
    M->S_dev_elems = s_elems;
  }
  LF_HIP(c, hipMemcpyAsync(M->S_dev, M->S_off.data(), ((size_t)q + 1) * sizeof(int), hipMemcpyHostToDevice, c->cur));
  if (!M->S_idx.empty())
    LF_HIP(c, hipMemcpyAsync(M->S_dev + q + 1, M->S_idx.data(), M->S_idx.size() * sizeof(int), hipMemcpyHostToDevice,
                             c->cur));
  LF_HIP(c, hipStreamSynchronize(c->cur));
  M->structured = true;
  return LF_OK;
}

// the largest pair of reordered ring-valued entry copies lf_ccs_create keeps (CcsDev::vh / vc):
// LATTICEUM_AMD_CCS_REORDER_BYTES in decimal bytes (0: no copies), read on every call
constexpr size_t CCS_REORDER_BYTES = (size_t)16 << 30;
static size_t ccs_reorder_bytes() {
  const char *e = getenv("LATTICEUM_AMD_CCS_REORDER_BYTES");
  if (!e || !*e) return CCS_REORDER_BYTES;
  char *end = nullptr;
  const unsigned long long v = strtoull(e, &end, 10);
  return *end ? CCS_REORDER_BYTES : (size_t)v;
}

int lf_ccs_create(lf_ctx *c, int d, int t, size_t m, size_t n, const uint64_t *row_ptr, const uint32_t *col,
                  const uint64_t *val, int repr, lf_ccs **out) {
  if (!c || !out || t < 1 || !m || !n || !row_ptr) return LF_ERR_INVALID_ARG;
  DevGuard g(c);
  LF_TRY(check_repr(c, repr));
  if (!ring_ok(d)) return fail(c, LF_ERR_UNSUPPORTED_RING, "unsupported ring degree");
  *out = nullptr;
  const size_t nnz = row_ptr[(size_t)t * (m + 1) - 1];
  if (nnz >= (1ull << 32) || (nnz && (!col || !val)) || (size_t)t * n >= (1ull << 32))
    return fail(c, LF_ERR_INVALID_ARG, "CCS: nnz and t n must fit 32-bit indices");
  for (int j = 0; j < t; j++) {
    const uint64_t *rp = row_ptr + (size_t)j * (m + 1);
    for (size_t r = 0; r < m; r++)
      if (rp[r] > rp[r + 1]) return fail(c, LF_ERR_INVALID_ARG, "CCS: row offsets must not decrease");
    if (j && rp[0] != row_ptr[(size_t)j * (m + 1) - 1]) return fail(c, LF_ERR_INVALID_ARG, "CCS: matrices must be contiguous");
  }
  for (size_t k = 0; k < nnz; k++)
    if (col[k] >= n) return fail(c, LF_ERR_INVALID_ARG, "CCS: column index out of range");
  // the row-merged matrix (SparseMatrix::hconcat) and the per-matrix transposes
  std::vector<uint64_t> hrp(m + 1, 0), crp((size_t)t * (n + 1), 0);
  std::vector<uint32_t> hcol(nnz), hidx(nnz), crow(nnz), cidx(nnz);
  for (int j = 0; j < t; j++)
    for (size_t r = 0; r < m; r++) hrp[r + 1] += row_ptr[(size_t)j * (m + 1) + r + 1] - row_ptr[(size_t)j * (m + 1) + r];
  for (size_t r = 0; r < m; r++) hrp[r + 1] += hrp[r];
  {
    std::vector<uint64_t> fill(hrp.begin(), hrp.end() - 1);
    for (size_t r = 0; r < m; r++)
      for (int j = 0; j < t; j++)
        for (uint64_t k = row_ptr[(size_t)j * (m + 1) + r]; k < row_ptr[(size_t)j * (m + 1) + r + 1]; k++) {
          hcol[fill[r]] = (uint32_t)(j * n + col[k]);
          hidx[fill[r]++] = (uint32_t)k;
        }
  }
  for (int j = 0; j < t; j++) {
    uint64_t *cp = crp.data() + (size_t)j * (n + 1);
    const uint64_t *rp = row_ptr + (size_t)j * (m + 1);
    for (uint64_t k = rp[0]; k < rp[m]; k++) cp[col[k] + 1]++;
    cp[0] = rp[0];
    for (size_t q = 0; q < n; q++) cp[q + 1] += cp[q];
    std::vector<uint64_t> fill(cp, cp + n);
    for (size_t r = 0; r < m; r++)
      for (uint64_t k = rp[r]; k < rp[r + 1]; k++) {
        crow[fill[col[k]]] = (uint32_t)r;
        cidx[fill[col[k]]++] = (uint32_t)k;
      }
  }
  auto M = std::make_unique<lf_ccs>();
  M->device = c->device;
  M->live.resize((size_t)t * m);
  for (int j = 0; j < t; j++)
    for (size_t r = 0; r < m; r++)
      M->live[(size_t)j * m + r] = row_ptr[(size_t)j * (m + 1) + r + 1] > row_ptr[(size_t)j * (m + 1) + r];
  auto put = [&](const void *h, size_t bytes, void **dst) -> int {
    LF_HIP(c, hipMalloc(dst, bytes ? bytes : 8));
    M->bufs.push_back(*dst);
    if (bytes) LF_HIP(c, hipMemcpyAsync(*dst, h, bytes, hipMemcpyHostToDevice, c->cur));
    return LF_OK;
  };
  void *p;
  lfk::CcsDev &D = M->dev;
  D.d = d;
  D.t = t;
  D.m = m;
  D.n = n;
  LF_TRY(put(row_ptr, (size_t)t * (m + 1) * 8, &p));
  D.rp = (const uint64_t *)p;
  LF_TRY(put(col, nnz * 4, &p));
  D.col = (const uint32_t *)p;
  LF_TRY(put(val, nnz * d * 8, &p));
  D.val = (const uint64_t *)p;
  if (repr == LF_REPR_MONTGOMERY && nnz) LF_HIP(c, lfk::mont((uint64_t *)p, nnz * d, false, c->cur));
  {  // every entry a scalar (its value in word 0 of each slot, zero elsewhere: from_scalar,
     // ntt_form.rs:689-692)? then the products read one word per entry (CcsDev::sval)
    const int tb = lfk::slot_words(d);
    bool scalar = nnz > 0;
    for (size_t k = 0; k < nnz && scalar; k++) {
      const uint64_t *v = val + k * d;
      for (int w = 0; w < d; w++)
        if (v[w] != (w % tb == 0 ? v[0] : 0)) {
          scalar = false;
          break;
        }
    }
    if (scalar) {
      // also in the row-merged and transposed orders, so those products read them
      // sequentially instead of gathering one word per entry through hidx / cidx
      std::vector<uint64_t> sv(nnz), sh(nnz), sc(nnz);
      for (size_t k = 0; k < nnz; k++) sv[k] = val[k * d];
      for (size_t k = 0; k < nnz; k++) {
        sh[k] = sv[hidx[k]];
        sc[k] = sv[cidx[k]];
      }
      const uint64_t **dst[3] = {&D.sval, &D.svh, &D.svc};
      const std::vector<uint64_t> *src[3] = {&sv, &sh, &sc};
      for (int q = 0; q < 3; q++) {
        LF_TRY(put(src[q]->data(), nnz * 8, &p));
        *dst[q] = (const uint64_t *)p;
        if (repr == LF_REPR_MONTGOMERY) LF_HIP(c, lfk::mont((uint64_t *)p, nnz, false, c->cur));
      }
      LF_HIP(c, hipStreamSynchronize(c->cur));  // the host vectors go out of scope
    }
  }
  LF_TRY(put(hrp.data(), hrp.size() * 8, &p));
  D.hrp = (const uint64_t *)p;
  LF_TRY(put(hcol.data(), nnz * 4, &p));
  D.hcol = (const uint32_t *)p;
  LF_TRY(put(hidx.data(), nnz * 4, &p));
  D.hidx = (const uint32_t *)p;
  LF_TRY(put(crp.data(), crp.size() * 8, &p));
  D.crp = (const uint64_t *)p;
  LF_TRY(put(crow.data(), nnz * 4, &p));
  D.crow = (const uint32_t *)p;
  LF_TRY(put(cidx.data(), nnz * 4, &p));
  D.cidx = (const uint32_t *)p;
  // ring-valued entries: copies in the row-merged and transposes' orders, so the
  // challenged pass and the Mz weights read their values sequentially instead of
  // gathering d words per entry through hidx / cidx (at the zkvm's shape 2 x 3.15 GB;
  // above ccs_reorder_bytes() the gathers stay). The copies are optional: when one
  // cannot be allocated, both are dropped and the products gather
  if (!D.sval && nnz && 2 * nnz * d * 8 <= ccs_reorder_bytes()) {
    const uint32_t *ix[2] = {D.hidx, D.cidx};
    void *cp[2] = {nullptr, nullptr};
    if (hipMalloc(&cp[0], nnz * d * 8) != hipSuccess || hipMalloc(&cp[1], nnz * d * 8) != hipSuccess) {
      (void)hipGetLastError();  // clear it: not this call's failure
      if (cp[0]) (void)hipFree(cp[0]);
      cp[0] = cp[1] = nullptr;
    }
    for (int q = 0; q < 2 && cp[0]; q++) M->bufs.push_back(cp[q]);
    for (int q = 0; q < 2 && cp[0]; q++)
      LF_HIP(c, lfk::gather_entries(D.val, ix[q], nnz, d, (uint64_t *)cp[q], c->cur));
    D.vh = (const uint64_t *)cp[0];
    D.vc = (const uint64_t *)cp[1];
  }
  LF_HIP(c, hipStreamSynchronize(c->cur));  // the host vectors go out of scope
  *out = M.release();
  return LF_OK;
}

static int mz_check(lf_ctx *c, const lf_ccs *M, int nz, int nv) {
  if (!M || nz < 1 || nv < 1) return fail(c, LF_ERR_INVALID_ARG, "CCS products: null matrices or no vectors");
  if (M->device != c->device) return fail(c, LF_ERR_INVALID_ARG, "CCS matrices live on another device");
  if (M->dev.m > ((size_t)1 << nv)) return fail(c, LF_ERR_INVALID_ARG, "MLE too short for m rows (to_mles_err)");
  return LF_OK;
}

int lf_dev_mz_mles(lf_ctx *c, const lf_ccs *M, const uint64_t *z, int nz, int nv, uint64_t *out) {
  if (!c || !z || !out) return LF_ERR_INVALID_ARG;
  DevGuard g(c);
  LF_TRY(mz_check(c, M, nz, nv));
  LF_HIP(c, lfk::mz_mles(M->dev, z, nz, nv, out, c->cur));
  return LF_OK;
}

int lf_dev_mz_mles_sel(lf_ctx *c, const lf_ccs *M, const uint64_t *z, const int *sel, int nsel, int nv,
                       uint64_t *out) {
  if (!c || !z || !out || (!sel && nsel) || nsel < 0) return LF_ERR_INVALID_ARG;
  DevGuard g(c);
  LF_TRY(mz_check(c, M, 1, nv));
  for (int i = 0; i < nsel; i++)
    if (sel[i] < 0 || sel[i] >= M->dev.t) return fail(c, LF_ERR_INVALID_ARG, "matrix index out of range");
  if (!nsel) return LF_OK;
  LF_TRY(grow(c, c->sel, c->sel_elems, (size_t)nsel));
  LF_HIP(c, hipMemcpyAsync(c->sel, sel, (size_t)nsel * sizeof(int), hipMemcpyHostToDevice, c->cur));
  LF_HIP(c, lfk::mz_mles(M->dev, z, 1, nv, out, c->cur, c->sel, nsel));
  return LF_OK;
}

int lf_dev_mz_challenged(lf_ctx *c, const lf_ccs *M, const uint64_t *z, const uint64_t *zeta, int nz, int nv,
                         uint64_t *out) {
  if (!c || !z || !zeta || !out) return LF_ERR_INVALID_ARG;
  DevGuard g(c);
  LF_TRY(mz_check(c, M, nz, nv));
  LF_TRY(grow(c, c->tmp, c->tmp_elems, lfk::mz_scratch_elems(M->dev, nz, nv)));
  LF_HIP(c, lfk::mz_challenged(M->dev, z, zeta, nz, nv, out, c->tmp, c->cur));
  return LF_OK;
}

int lf_dev_mz_challenged_pair(lf_ctx *c, const lf_ccs *M, const uint64_t *z0, const uint64_t *zeta0,
                              const uint64_t *z1, const uint64_t *zeta1, int nz, int nv, uint64_t *out0,
                              uint64_t *out1) {
  if (!c || !z0 || !zeta0 || !z1 || !zeta1 || !out0 || !out1) return LF_ERR_INVALID_ARG;
  DevGuard g(c);
  LF_TRY(mz_check(c, M, nz, nv));
  const lfk::CcsDev &D = M->dev;
  LF_TRY(grow(c, c->tmp, c->tmp_elems, 2 * lfk::mz_chall_elems(D, nz)));
  LF_HIP(c, lfk::mz_challenged_pair(D, z0, zeta0, z1, zeta1, nz, nv, out0, out1, c->tmp, c->cur));
  return LF_OK;
}

int lf_dev_mz_evaluate(lf_ctx *c, const lf_ccs *M, const uint64_t *z, int nz, int nv, const uint64_t *point,
                       uint64_t *out) {
  if (!c || !z || !point || !out) return LF_ERR_INVALID_ARG;
  DevGuard g(c);
  LF_TRY(mz_check(c, M, nz, nv));
  LF_TRY(grow(c, c->tmp, c->tmp_elems, lfk::mz_scratch_elems(M->dev, nz, nv)));
  LF_HIP(c, lfk::mz_evaluate(M->dev, z, nz, nv, point, out, c->tmp, c->cur));
  return LF_OK;
}

int lf_dev_mz_weights(lf_ctx *c, const lf_ccs *M, int nv, const uint64_t *eq, uint64_t *w) {
  if (!c || !eq || !w) return LF_ERR_INVALID_ARG;
  DevGuard g(c);
  LF_TRY(mz_check(c, M, 1, nv));
  LF_HIP(c, lfk::mz_weights(M->dev, eq, w, c->cur));
  return LF_OK;
}

int lf_dev_mz_dots(lf_ctx *c, const lf_ccs *M, const uint64_t *w, const uint64_t *z, int nz, uint64_t *out) {
  if (!c || !M || !w || !z || !out || nz < 1) return LF_ERR_INVALID_ARG;
  DevGuard g(c);
  LF_TRY(grow(c, c->tmp, c->tmp_elems, lfk::mz_dots_partial_elems(M->dev, nz)));
  LF_HIP(c, lfk::mz_dots(M->dev, w, z, nz, out, c->cur, c->tmp));
  return LF_OK;
}

size_t lf_ccs_weights_len(const lf_ccs *M) { return M ? (size_t)M->dev.t * M->dev.n * M->dev.d : 0; }

// ---------------------------------------------------------------- relation checks
int lf_dev_ccs_check_relation(lf_ctx *c, const lf_ccs *M, const uint64_t *z, int nz, uint64_t *resid,
                              int64_t *first_bad) {
  if (!c || !z || !first_bad) return LF_ERR_INVALID_ARG;
  DevGuard g(c);
  if (!M || nz < 1 || nz > 65535) return fail(c, LF_ERR_INVALID_ARG, "CCS relation: null matrices or nz outside 1..65535");
  if (M->device != c->device) return fail(c, LF_ERR_INVALID_ARG, "CCS matrices live on another device");
  if (!M->structured) return fail(c, LF_ERR_INVALID_ARG, "CCS relation: lf_ccs_set_structure first (c and the multisets)");
  const int q = (int)M->S_off.size() - 1;
  LF_TRY(grow(c, c->rel, c->rel_elems, (size_t)nz));
  LF_HIP(c, lfk::ccs_relation(M->dev, z, nz, M->c_dev, q, M->S_dev, M->S_dev + q + 1, resid, c->rel, c->cur));
  std::vector<uint64_t> fb(nz);
  LF_HIP(c, hipMemcpyAsync(fb.data(), c->rel, (size_t)nz * 8, hipMemcpyDeviceToHost, c->cur));
  LF_HIP(c, hipStreamSynchronize(c->cur));
  bool ok = true;
  for (int i = 0; i < nz; i++) {
    first_bad[i] = fb[i] == ~0ull ? -1 : (int64_t)fb[i];
    ok &= first_bad[i] < 0;
  }
  return ok ? LF_OK : LF_ERR_NOT_SATISFIED;
}

int lf_dev_ccs_row_evals(lf_ctx *c, const lf_ccs *M, const uint64_t *z, size_t row, uint64_t *out) {
  if (!c || !z || !out) return LF_ERR_INVALID_ARG;
  DevGuard g(c);
  if (!M) return fail(c, LF_ERR_INVALID_ARG, "CCS row values: null matrices");
  if (M->device != c->device) return fail(c, LF_ERR_INVALID_ARG, "CCS matrices live on another device");
  if (row >= M->dev.m) return fail(c, LF_ERR_INVALID_ARG, "CCS row values: row out of range");
  LF_HIP(c, lfk::ccs_row_evals(M->dev, z, row, out, c->cur));
  return LF_OK;
}

int lf_dev_linf_norm(lf_ctx *c, const uint64_t *x, size_t n, uint64_t *norm) {
  if (!c || !norm || (n && !x)) return LF_ERR_INVALID_ARG;
  DevGuard g(c);
  if ((uintptr_t)x & 7) return fail(c, LF_ERR_INVALID_ARG, "linf norm: the words must be 8-byte aligned");
  LF_TRY(grow(c, c->rel, c->rel_elems, (size_t)1));
  LF_HIP(c, lfk::linf_norm(x, n, c->rel, c->cur));
  LF_HIP(c, hipMemcpyAsync(norm, c->rel, 8, hipMemcpyDeviceToHost, c->cur));
  LF_HIP(c, hipStreamSynchronize(c->cur));
  return LF_OK;
}

}  // extern "C"
