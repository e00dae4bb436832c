// api_memtree.hip -- lf_memtree_*: the Merkle tree of VM memory kept on the device
// between memory ops (include/lf.h). The handle owns a host mirror of the words and
// the node array in merkle_tree()'s layout; apply() walks a batch of ops on the
// mirror, snapshots every touched page, builds the batch's dependency tables on the
// host and runs lfk::memtree_apply (merkle.hip): one upload, depth + 2 launches, one
// download per chunk of ops.
#include <algorithm>
#include <memory>
#include <unordered_map>

#include "api_internal.hpp"

namespace {

// ops per internal chunk: bounds the device scratch to about MEMTREE_CHUNK x
// (words_per_page x 4 + (2 depth + 1) x 32) bytes (8 MB at 8192 x 256, and 6 MB of
// pinned host memory) while 4096 8-lane groups still give every layer launch 512 waves
constexpr size_t MEMTREE_CHUNK = 4096;

// prev / last of lf_memtree_plan. slot(l, node) is layer l's last-writer map: 1 + the
// latest op under that node so far, 0 for none; the caller hands it over all zero
template <class Slot>
void plan_tables(int depth, const uint32_t *pg, size_t k, Slot &&slot, int32_t *prev, uint8_t *last) {
  for (int l = 0; l <= depth; l++) {
    for (size_t j = 0; j < k; j++) {
      const uint64_t node = (uint64_t)pg[j] >> l;
      if (l < depth) prev[j * depth + l] = slot(l, node ^ 1) - 1;
      slot(l, node) = (int32_t)j + 1;
    }
    // after the pass the map holds every node's last op
    for (size_t j = 0; j < k; j++) last[j * (depth + 1) + l] = slot(l, (uint64_t)pg[j] >> l) == (int32_t)j + 1;
  }
}

}  // namespace

struct lf_memtree {
  lf_ctx *ctx = nullptr;
  int device = 0;
  size_t pages = 0, wpp = 0;
  int wbits = 0, depth = 0;
  size_t off[lfk::MEMTREE_MAX_DEPTH + 1] = {};
  std::vector<uint32_t> mem;     // the host mirror
  std::vector<int32_t> writer;   // plan_tables' maps, one slot per node, zero between calls
  uint64_t *nodes = nullptr;     // device: merkle_nodes(pages) x 4
  uint64_t root[4] = {};
  bool broken = false;           // a device call failed after the mirror moved on
  // per-chunk scratch for `cap` ops: [snapshots | page index | prev | last] up, [ver | paths] down
  size_t cap = 0;
  uint8_t *h_in = nullptr, *d_in = nullptr;
  uint64_t *h_out = nullptr, *d_out = nullptr;

  size_t in_bytes(size_t k) const { return k * (wpp * 4 + 4 + (size_t)depth * 4 + (size_t)depth + 1); }
  size_t ver_elems(size_t k) const { return (size_t)(depth + 1) * k * 4; }
  size_t out_elems(size_t k) const { return ver_elems(k) + k * (size_t)depth * 4; }
  void release_scratch() {
    if (h_in) (void)hipHostFree(h_in);
    if (h_out) (void)hipHostFree(h_out);
    if (d_in) (void)hipFree(d_in);
    if (d_out) (void)hipFree(d_out);
    h_in = d_in = nullptr;
    h_out = d_out = nullptr;
    cap = 0;
  }
  ~lf_memtree() {
    DevGuard g(device);
    release_scratch();
    if (nodes) (void)hipFree(nodes);
  }
};

static int memtree_reserve(lf_memtree *t, size_t k) {
  if (k <= t->cap) return LF_OK;
  lf_ctx *c = t->ctx;
  t->release_scratch();
  LF_HIP(c, hipHostMalloc((void **)&t->h_in, t->in_bytes(k), hipHostMallocDefault));
  LF_HIP(c, hipHostMalloc((void **)&t->h_out, (k * 4 + k * (size_t)t->depth * 4 + 1) * 8, hipHostMallocDefault));
  LF_HIP(c, hipMalloc((void **)&t->d_in, t->in_bytes(k)));
  LF_HIP(c, hipMalloc((void **)&t->d_out, t->out_elems(k) * 8));
  t->cap = k;
  return LF_OK;
}

// the shape of a memory: at least one page of a power-of-two number of words, every
// word with a 32-bit byte address -> log2(words_per_page)
static int memtree_shape(lf_ctx *c, size_t pages, size_t words_per_page, int &wbits) {
  wbits = words_per_page == 1 ? 0 : log2_exact(words_per_page);
  if (!pages || wbits < 0)
    return fail(c, LF_ERR_INVALID_ARG, "memtree: at least one page of a power-of-two number of words");
  if (wbits > 30 || pages > ((size_t)1 << (30 - wbits)))
    return fail(c, LF_ERR_INVALID_ARG, "memtree: the memory exceeds the 32-bit address space");
  return LF_OK;
}

int lf_memtree_create(lf_ctx *c, const uint32_t *words, size_t pages, size_t words_per_page, lf_memtree **out) {
  if (!c || !out) return LF_ERR_INVALID_ARG;
  *out = nullptr;
  if (!words) return fail(c, LF_ERR_INVALID_ARG, "memtree: at least one page of a power-of-two number of words");
  int wbits;
  LF_TRY(memtree_shape(c, pages, words_per_page, wbits));
  DevGuard g(c);
  auto t = std::make_unique<lf_memtree>();
  t->ctx = c;
  t->device = c->device;
  t->pages = pages;
  t->wpp = words_per_page;
  t->wbits = wbits;
  t->depth = lfk::merkle_layer_offsets(pages, t->off, lfk::MEMTREE_MAX_DEPTH + 1);
  if (t->depth < 0) return fail(c, LF_ERR_INVALID_ARG, "memtree: too many pages");
  const size_t nw = pages * words_per_page, nn = lfk::merkle_nodes(pages);
  t->mem.assign(words, words + nw);
  t->writer.assign(nn, 0);
  LF_HIP(c, hipMalloc((void **)&t->nodes, nn * 32));
  {
    // the one full build; the device copy of the memory is dropped afterwards
    std::vector<uint64_t> wide(words, words + nw);
    DevBuf rows;
    LF_TRY(upload(c, rows, wide.data(), nw, LF_REPR_CANONICAL));
    LF_HIP(c, lfk::merkle_tree(rows.p, pages, words_per_page, t->nodes, c->cur));
    LF_HIP(c, hipMemcpyAsync(t->root, t->nodes + 4 * (nn - 1), 32, hipMemcpyDeviceToHost, c->cur));
    LF_HIP(c, hipStreamSynchronize(c->cur));
  }
  *out = t.release();
  return LF_OK;
}

void lf_memtree_destroy(lf_memtree *t) { delete t; }

int lf_memtree_root(const lf_memtree *t, uint64_t out4[4]) {
  if (!t || !out4) return LF_ERR_INVALID_ARG;
  memcpy(out4, t->root, 32);
  return LF_OK;
}

size_t lf_memtree_depth(const lf_memtree *t) { return t ? (size_t)t->depth : 0; }
size_t lf_memtree_chunk(void) { return MEMTREE_CHUNK; }
const uint64_t *lf_memtree_nodes_device(const lf_memtree *t) { return t ? t->nodes : nullptr; }

int lf_memtree_nodes_host(const lf_memtree *t, uint64_t *out) {
  if (!t || !out) return LF_ERR_INVALID_ARG;
  lf_ctx *c = t->ctx;
  DevGuard g(c);
  LF_HIP(c, hipMemcpyAsync(out, t->nodes, lfk::merkle_nodes(t->pages) * 32, hipMemcpyDeviceToHost, c->cur));
  LF_HIP(c, hipStreamSynchronize(c->cur));
  return LF_OK;
}

// one chunk of k <= MEMTREE_CHUNK validated ops
static int memtree_chunk(lf_memtree *t, const lf_mem_op *ops, size_t k, uint64_t *roots, uint32_t *pages_out,
                         uint64_t *paths, uint32_t *page_index) {
  lf_ctx *c = t->ctx;
  const size_t wpp = t->wpp, depth = (size_t)t->depth;
  LF_TRY(memtree_reserve(t, k));
  uint32_t *snap = reinterpret_cast<uint32_t *>(t->h_in), *pg = snap + k * wpp;
  int32_t *prev = reinterpret_cast<int32_t *>(pg + k);
  uint8_t *last = reinterpret_cast<uint8_t *>(prev + k * depth);
  for (size_t j = 0; j < k; j++) {
    const size_t word = ops[j].address >> 2, page = word >> t->wbits;
    if (ops[j].is_write) t->mem[word] = ops[j].value;
    memcpy(snap + j * wpp, t->mem.data() + page * wpp, wpp * 4);
    pg[j] = (uint32_t)page;
  }
  plan_tables(t->depth, pg, k, [t](int l, uint64_t node) -> int32_t & { return t->writer[t->off[l] + node]; }, prev,
              last);
  for (size_t j = 0; j < k; j++)
    for (size_t l = 0; l <= depth; l++) t->writer[t->off[l] + ((size_t)pg[j] >> l)] = 0;
  if (pages_out) memcpy(pages_out, snap, k * wpp * 4);
  if (page_index) memcpy(page_index, pg, k * 4);

  // from here on a failure leaves the mirror ahead of the device tree
  t->broken = true;
  lfk::MemtreeBatch b;
  b.pages = reinterpret_cast<const uint32_t *>(t->d_in);
  b.pg = b.pages + k * wpp;
  b.prev = reinterpret_cast<const int32_t *>(b.pg + k);
  b.last = reinterpret_cast<const uint8_t *>(b.prev + k * depth);
  b.ver = t->d_out;
  b.paths = t->d_out + t->ver_elems(k);
  LF_HIP(c, hipMemcpyAsync(t->d_in, t->h_in, t->in_bytes(k), hipMemcpyHostToDevice, c->cur));
  LF_HIP(c, lfk::memtree_apply(t->nodes, t->pages, wpp, b, k, c->cur));
  // ver[depth] (the roots) and the paths are adjacent: one transfer
  LF_HIP(c, hipMemcpyAsync(t->h_out, b.ver + depth * k * 4, (k * 4 + k * depth * 4) * 8, hipMemcpyDeviceToHost,
                           c->cur));
  LF_HIP(c, hipStreamSynchronize(c->cur));
  t->broken = false;
  memcpy(roots, t->h_out, k * 32);
  if (paths) memcpy(paths, t->h_out + k * 4, k * depth * 32);
  memcpy(t->root, t->h_out + (k - 1) * 4, 32);
  return LF_OK;
}

int lf_memtree_apply(lf_memtree *t, const lf_mem_op *ops, size_t k, uint64_t *roots, uint32_t *pages_out,
                     uint64_t *paths, uint32_t *page_index) {
  if (!t) return LF_ERR_INVALID_ARG;
  lf_ctx *c = t->ctx;
  if (t->broken) return fail(c, LF_ERR_DEVICE, "memtree: an earlier apply failed on the device; rebuild the handle");
  if (!k) return LF_OK;
  if (!ops || !roots) return fail(c, LF_ERR_INVALID_ARG, "memtree: ops and roots are required");
  for (size_t j = 0; j < k; j++)
    if (((size_t)(ops[j].address >> 2) >> t->wbits) >= t->pages)
      return fail(c, LF_ERR_INVALID_ARG, "memtree: op " + std::to_string(j) + " addresses past the memory");
  DevGuard g(c);
  for (size_t at = 0; at < k; at += MEMTREE_CHUNK) {
    const size_t kc = std::min(MEMTREE_CHUNK, k - at);
    LF_TRY(memtree_chunk(t, ops + at, kc, roots + at * 4, pages_out ? pages_out + at * t->wpp : nullptr,
                         paths ? paths + at * (size_t)t->depth * 4 : nullptr, page_index ? page_index + at : nullptr));
  }
  return LF_OK;
}

int lf_memtree_plan(size_t pages, const uint32_t *page_of_op, size_t k, int32_t *prev, uint8_t *last) {
  size_t off[lfk::MEMTREE_MAX_DEPTH + 2];
  const int depth = pages ? lfk::merkle_layer_offsets(pages, off, lfk::MEMTREE_MAX_DEPTH + 2) : -1;
  if (depth < 0 || k > (size_t)INT32_MAX || (k && (!page_of_op || !last || (depth && !prev))))
    return LF_ERR_INVALID_ARG;
  for (size_t j = 0; j < k; j++)
    if (page_of_op[j] >= pages) return LF_ERR_INVALID_ARG;
  std::vector<std::unordered_map<uint64_t, int32_t>> maps(depth + 1);
  plan_tables(depth, page_of_op, k, [&maps](int l, uint64_t node) -> int32_t & { return maps[l][node]; }, prev, last);
  return LF_OK;
}

// ---------------------------------------------------------------- checking records
namespace {

// one chunk of k records and ntask (k or 2k) checks, in the context's pinned buffer and
// its device copy: [roots ntask x 4 | paths k x depth x 4 | rows ntask x wpp u32 |
// index k u32 | status ntask bytes]
struct CheckLayout {
  size_t paths, rows, index, ok, bytes;
  CheckLayout(size_t k, size_t ntask, size_t wpp, size_t depth) {
    paths = ntask * 32;
    rows = paths + k * depth * 32;
    index = rows + ntask * wpp * 4;
    ok = (index + k * 4 + 7) & ~(size_t)7;
    bytes = ok + ntask;
  }
};

int check_reserve(lf_ctx *c, size_t bytes) {
  if (bytes <= c->mv_bytes) return LF_OK;
  if (c->mv_host) (void)hipHostFree(c->mv_host);
  if (c->mv_dev) (void)hipFree(c->mv_dev);
  c->mv_host = c->mv_dev = nullptr;
  c->mv_bytes = 0;
  LF_HIP(c, hipHostMalloc((void **)&c->mv_host, bytes, hipHostMallocDefault));
  LF_HIP(c, hipMalloc((void **)&c->mv_dev, bytes));
  c->mv_bytes = bytes;
  return LF_OK;
}

// the staged chunk up, its ntask checks, the status bytes back into the pinned buffer
int check_run(lf_ctx *c, const CheckLayout &L, size_t k, size_t ntask, size_t pages, size_t wpp) {
  uint8_t *d = c->mv_dev;
  LF_HIP(c, hipMemcpyAsync(d, c->mv_host, L.ok, hipMemcpyHostToDevice, c->cur));
  LF_HIP(c, lfk::merkle_verify(reinterpret_cast<const uint32_t *>(d + L.rows), ntask, k, wpp, pages,
                               reinterpret_cast<const uint32_t *>(d + L.index),
                               reinterpret_cast<const uint64_t *>(d + L.paths), reinterpret_cast<const uint64_t *>(d),
                               false, d + L.ok, c->cur));
  LF_HIP(c, hipMemcpyAsync(c->mv_host + L.ok, d + L.ok, ntask, hipMemcpyDeviceToHost, c->cur));
  LF_HIP(c, hipStreamSynchronize(c->cur));
  return LF_OK;
}

bool same_digest(const uint64_t *a, const uint64_t *b) {
  for (int w = 0; w < 4; w++)
    if (gl::canon(a[w]) != gl::canon(b[w])) return false;
  return true;
}

}  // namespace

int lf_memtree_verify(lf_ctx *c, size_t pages, size_t words_per_page, size_t k, const uint64_t *roots,
                      const uint32_t *pages_in, const uint64_t *paths, const uint32_t *page_index,
                      int64_t *first_bad) {
  if (!c || !first_bad) return LF_ERR_INVALID_ARG;
  *first_bad = -1;
  int wbits;
  LF_TRY(memtree_shape(c, pages, words_per_page, wbits));
  if (!k) return LF_OK;
  const size_t wpp = words_per_page, depth = (size_t)lfk::merkle_depth(pages);
  if (!roots || !pages_in || !page_index || (depth && !paths))
    return fail(c, LF_ERR_INVALID_ARG, "memtree verify: roots, pages, paths and page indices are required");
  DevGuard g(c);
  for (size_t at = 0; at < k; at += MEMTREE_CHUNK) {
    const size_t kc = std::min(MEMTREE_CHUNK, k - at);
    const CheckLayout L(kc, kc, wpp, depth);
    LF_TRY(check_reserve(c, L.bytes));
    uint8_t *h = c->mv_host;
    memcpy(h, roots + at * 4, kc * 32);
    if (depth) memcpy(h + L.paths, paths + at * depth * 4, kc * depth * 32);
    memcpy(h + L.rows, pages_in + at * wpp, kc * wpp * 4);
    memcpy(h + L.index, page_index + at, kc * 4);
    LF_TRY(check_run(c, L, kc, kc, pages, wpp));
    for (size_t j = 0; j < kc; j++)
      if (!h[L.ok + j]) {
        *first_bad = (int64_t)(at + j);
        return fail(c, LF_ERR_VERIFICATION,
                    "memtree verify: record " + std::to_string(at + j) + " does not open its root");
      }
  }
  return LF_OK;
}

int lf_memtree_audit(lf_ctx *c, size_t pages, size_t words_per_page, const uint64_t start_root[4],
                     const lf_mem_op *ops, const uint32_t *old_words, size_t k, const uint64_t *roots,
                     const uint32_t *pages_in, const uint64_t *paths, const uint32_t *page_index, int64_t *first_bad,
                     int *failed) {
  if (!c || !first_bad || !failed) return LF_ERR_INVALID_ARG;
  *first_bad = -1;
  *failed = LF_MEMLOG_OK;
  int wbits;
  LF_TRY(memtree_shape(c, pages, words_per_page, wbits));
  if (!k) return LF_OK;
  const size_t wpp = words_per_page, depth = (size_t)lfk::merkle_depth(pages);
  if (!start_root || !ops || !roots || !pages_in || !page_index || (depth && !paths))
    return fail(c, LF_ERR_INVALID_ARG,
                "memtree audit: the start root, ops, roots, pages, paths and page indices are required");
  if (!old_words)
    for (size_t j = 0; j < k; j++)
      if (ops[j].is_write) return fail(c, LF_ERR_INVALID_ARG, "memtree audit: a log with writes needs old_words");
  DevGuard g(c);
  for (size_t at = 0; at < k; at += MEMTREE_CHUNK) {
    const size_t kc = std::min(MEMTREE_CHUNK, k - at);
    // task j: the page after op at + j against its root; task kc + j: the page before it
    // (the written word set back) against the root before it, under the same path
    const CheckLayout L(kc, 2 * kc, wpp, depth);
    LF_TRY(check_reserve(c, L.bytes));
    uint8_t *h = c->mv_host;
    const uint64_t *before = at ? roots + (at - 1) * 4 : start_root;
    memcpy(h, roots + at * 4, kc * 32);
    memcpy(h + kc * 32, before, 32);
    memcpy(h + kc * 32 + 32, roots + at * 4, (kc - 1) * 32);
    if (depth) memcpy(h + L.paths, paths + at * depth * 4, kc * depth * 32);
    uint32_t *post = reinterpret_cast<uint32_t *>(h + L.rows), *pre = post + kc * wpp;
    memcpy(post, pages_in + at * wpp, kc * wpp * 4);
    memcpy(pre, post, kc * wpp * 4);
    for (size_t j = 0; j < kc; j++)
      if (ops[at + j].is_write) pre[j * wpp + ((ops[at + j].address >> 2) & (wpp - 1))] = old_words[at + j];
    memcpy(h + L.index, page_index + at, kc * 4);
    LF_TRY(check_run(c, L, kc, 2 * kc, pages, wpp));
    const uint8_t *ok_post = h + L.ok, *ok_pre = ok_post + kc;
    for (size_t j = 0; j < kc; j++) {
      const lf_mem_op &op = ops[at + j];
      const size_t word = op.address >> 2, page = word >> wbits;
      int bad = LF_MEMLOG_OK;
      if (page >= pages || page_index[at + j] != page)
        bad = LF_MEMLOG_INDEX;
      else if (op.is_write && pages_in[(at + j) * wpp + (word & (wpp - 1))] != op.value)
        bad = LF_MEMLOG_VALUE;
      else if (!ok_post[j])
        bad = LF_MEMLOG_OPENING;
      else if (op.is_write ? !ok_pre[j] : !same_digest(roots + (at + j) * 4, j ? roots + (at + j - 1) * 4 : before))
        bad = LF_MEMLOG_TRANSITION;
      if (bad) {
        *first_bad = (int64_t)(at + j);
        *failed = bad;
        return fail(c, LF_ERR_VERIFICATION,
                    "memtree audit: op " + std::to_string(at + j) + " fails check " + std::to_string(bad));
      }
    }
  }
  return LF_OK;
}
