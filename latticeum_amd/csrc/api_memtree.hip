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

int lf_memtree_create(lf_ctx *c, const uint32_t *words, size_t pages, size_t words_per_page, lf_memtree **out) {
  if (!c || !out) return LF_ERR_INVALID_ARG;
  *out = nullptr;
  const int wbits = words_per_page == 1 ? 0 : log2_exact(words_per_page);
  if (!words || !pages || wbits < 0)
    return fail(c, LF_ERR_INVALID_ARG, "memtree: at least one page of a power-of-two number of words");
  // every word has a 32-bit byte address
  if (wbits > 30 || pages > ((size_t)1 << (30 - wbits)))
    return fail(c, LF_ERR_INVALID_ARG, "memtree: the memory exceeds the 32-bit address space");
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
