// merkle.hip -- width-8 Poseidon2 Merkle trees of VM memory (SURVEY.md 8(f)
// rank 3): the zkvm's ZkVmCommitter hashes every memory page (a row of the
// memory matrix) with PaddingFreeSponge<Poseidon2Goldilocks<8>, 8, 4, 4> and
// joins digests with TruncatedPermutation<.., 2, 4, 8> up to the root
// (zkvm/src/commitments.rs:192-262, poseidon2.rs:31-49). Every page hash is an
// independent sponge chain (one thread each); every tree level is one launch
// of independent compressions.
//
// One permutation state spreads over 8 lanes (permute8_lane) in the tree
// kernels; the batched permutation keeps one state per thread.
//
// Constants: the width-8 external rounds from the reference
// (crypto_consts.rs:9-96), the 22 internal constants shared with width 16;
// the internal diagonal is Plonky3's MATRIX_DIAG_8_GOLDILOCKS, which the
// reference does not vendor (restated; parity unpinned).
#include "gl.hpp"
#include "kernels.hpp"
#include "launch.hpp"
#include "p2_consts.inc"

namespace lfk {

namespace {

__constant__ uint64_t W8_EXT_INIT[32] = LF_P2W8_EXT_INIT;
__constant__ uint64_t W8_EXT_TERM[32] = LF_P2W8_EXT_TERM;
__constant__ uint64_t W8_INTERNAL[22] = LF_P2_INTERNAL;
__constant__ uint64_t W8_DIAG_M1[8] = LF_P2W8_DIAG_M1;

__device__ __forceinline__ uint64_t sbox7(uint64_t x) {
  const uint64_t x2 = gl::mul(x, x), x4 = gl::mul(x2, x2);
  return gl::mul(gl::mul(x4, x2), x);
}
// MDS light (poseidon2.rs:243-268 at width 8): MDSMat4 on each 4-chunk, then
// each word plus the sum of its column over the chunks
__device__ __forceinline__ void mds8(uint64_t *s) {
#pragma unroll
  for (int c = 0; c < 8; c += 4) {
    const uint64_t x0 = s[c], x1 = s[c + 1], x2 = s[c + 2], x3 = s[c + 3];
    const uint64_t t = gl::add(gl::add(x0, x1), gl::add(x2, x3));
    s[c + 0] = gl::add(t, gl::add(x0, gl::add(x1, x1)));
    s[c + 1] = gl::add(t, gl::add(x1, gl::add(x2, x2)));
    s[c + 2] = gl::add(t, gl::add(x2, gl::add(x3, x3)));
    s[c + 3] = gl::add(t, gl::add(x3, gl::add(x0, x0)));
  }
#pragma unroll
  for (int k = 0; k < 4; k++) {
    const uint64_t sum = gl::add(s[k], s[4 + k]);
    s[k] = gl::add(s[k], sum);
    s[4 + k] = gl::add(s[4 + k], sum);
  }
}
__device__ void permute8(uint64_t *s) {
  mds8(s);
#pragma unroll 1
  for (int r = 0; r < 4; r++) {
#pragma unroll
    for (int i = 0; i < 8; i++) s[i] = sbox7(gl::add(s[i], W8_EXT_INIT[8 * r + i]));
    mds8(s);
  }
#pragma unroll 1
  for (int r = 0; r < 22; r++) {
    s[0] = sbox7(gl::add(s[0], W8_INTERNAL[r]));
    uint64_t sum = 0;
#pragma unroll
    for (int i = 0; i < 8; i++) sum = gl::add(sum, s[i]);
#pragma unroll
    for (int i = 0; i < 8; i++) s[i] = gl::add(gl::mul(s[i], W8_DIAG_M1[i]), sum);
  }
#pragma unroll 1
  for (int r = 0; r < 4; r++) {
#pragma unroll
    for (int i = 0; i < 8; i++) s[i] = sbox7(gl::add(s[i], W8_EXT_TERM[8 * r + i]));
    mds8(s);
  }
}

__global__ void __launch_bounds__(256) k_p2w8_permute(uint64_t *states, size_t n) {
  const size_t e = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
  if (e >= n) return;
  uint64_t s[8];
#pragma unroll
  for (int i = 0; i < 8; i++) s[i] = gl::canon(states[e * 8 + i]);
  permute8(s);
#pragma unroll
  for (int i = 0; i < 8; i++) states[e * 8 + i] = s[i];
}

// ---------------------------------------------------------------- one state over 8 lanes
// A sponge chain is sequential, so a tree over P pages has only P independent
// chains (8 MB of memory: 8192, an eighth of the chip's SIMDs at one lane
// each). Here lane i of an 8-lane group holds state word i: the s-boxes of a
// full round run in parallel, the MDS mixing and the partial rounds' sum use
// cross-lane reads (ds_swizzle / bpermute), and 8x as many waves run.
__device__ __forceinline__ uint64_t shfl64(uint64_t x, int src) {
  const uint32_t lo = (uint32_t)__shfl((int)(uint32_t)x, src), hi = (uint32_t)__shfl((int)(uint32_t)(x >> 32), src);
  return (uint64_t)lo | ((uint64_t)hi << 32);
}
__device__ __forceinline__ uint64_t shfl64_xor(uint64_t x, int m) {
  const uint32_t lo = (uint32_t)__shfl_xor((int)(uint32_t)x, m), hi = (uint32_t)__shfl_xor((int)(uint32_t)(x >> 32), m);
  return (uint64_t)lo | ((uint64_t)hi << 32);
}
// mds8 with word i in lane i of the group (lane = the thread's lane in the wave)
__device__ __forceinline__ uint64_t mds8_lane(uint64_t x, int lane) {
  const uint64_t s1 = gl::add(x, shfl64_xor(x, 1));
  const uint64_t t = gl::add(s1, shfl64_xor(s1, 2));                 // the 4-chunk's sum
  const uint64_t xn = shfl64(x, (lane & ~3) | ((lane + 1) & 3));     // x_(i+1 mod 4) of the chunk
  const uint64_t y = gl::add(t, gl::add(x, gl::add(xn, xn)));
  return gl::add(y, gl::add(y, shfl64_xor(y, 4)));                   // + the column sum over the two chunks
}
__device__ uint64_t permute8_lane(uint64_t x, int lane) {
  const int i = lane & 7;
  x = mds8_lane(x, lane);
#pragma unroll 1
  for (int r = 0; r < 4; r++) x = mds8_lane(sbox7(gl::add(x, W8_EXT_INIT[8 * r + i])), lane);
  const uint64_t dg = W8_DIAG_M1[i];
#pragma unroll 1
  for (int r = 0; r < 22; r++) {
    if (i == 0) x = sbox7(gl::add(x, W8_INTERNAL[r]));
    uint64_t sum = gl::add(x, shfl64_xor(x, 1));
    sum = gl::add(sum, shfl64_xor(sum, 2));
    sum = gl::add(sum, shfl64_xor(sum, 4));
    x = gl::add(gl::mul(x, dg), sum);
  }
#pragma unroll 1
  for (int r = 0; r < 4; r++) x = mds8_lane(sbox7(gl::add(x, W8_EXT_TERM[8 * r + i])), lane);
  return x;
}

// leaf e = PaddingFreeSponge hash of row e: overwrite state[0..4) with the next
// four words, permute; a partial last block is permuted too; no padding. One
// 8-lane group per row (groups past nrows run on a clamped row, store nothing:
// every lane of a wave takes part in the cross-lane reads)
__global__ void __launch_bounds__(256) k_merkle_leaves(const uint64_t *rows, size_t nrows, size_t width,
                                                      uint64_t *leaves) {
  const size_t t = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
  const int lane = threadIdx.x & 63, i = lane & 7;
  const size_t e = t >> 3;
  const bool ok = e < nrows;
  const uint64_t *row = rows + (ok ? e : 0) * width;
  uint64_t x = 0;
  for (size_t pos = 0; pos < width; pos += 4) {
    const size_t take = width - pos < 4 ? width - pos : 4;
    if ((size_t)i < take) x = gl::canon(row[pos + i]);
    x = permute8_lane(x, lane);
  }
  if (ok && i < 4) leaves[e * 4 + i] = x;
}

// parent e = permute(child 2e || child 2e + 1)[0..4): the 8 words are contiguous
__global__ void __launch_bounds__(256) k_merkle_level(const uint64_t *children, size_t nparents, uint64_t *parents) {
  const size_t t = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
  const int lane = threadIdx.x & 63, i = lane & 7;
  const size_t e = t >> 3;
  const bool ok = e < nparents;
  uint64_t x = children[(ok ? e : 0) * 8 + i];
  x = permute8_lane(x, lane);
  if (ok && i < 4) parents[e * 4 + i] = x;
}

// ---------------------------------------------------------------- persistent memory tree
// A batch of k memory ops against a tree that stays on the device (lf_memtree_*):
// op j carries the snapshot of its page after ops 0..j, and ver[l][j] is the digest
// of the node above that page in layer l after ops 0..j. The sibling a layer needs
// is the version of the latest earlier op under the sibling node (prev), else the
// base tree's node, which the layer launches only read.
//
// ver[0][j] = the sponge of snapshot j (u32 words; k_merkle_leaves' partial last block)
__global__ void __launch_bounds__(256) k_memtree_leaves(const uint32_t *pages, size_t k, size_t width,
                                                       uint64_t *ver0) {
  const size_t t = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
  const int lane = threadIdx.x & 63, i = lane & 7;
  const size_t e = t >> 3;
  const bool ok = e < k;
  const uint32_t *row = pages + (ok ? e : 0) * width;
  uint64_t x = 0;
  for (size_t pos = 0; pos < width; pos += 4) {
    const size_t take = width - pos < 4 ? width - pos : 4;
    if ((size_t)i < take) x = row[pos + i];
    x = permute8_lane(x, lane);
  }
  if (ok && i < 4) ver0[e * 4 + i] = x;
}

// ver[l + 1][j] = permute(left || right)[0..4) of ver[l][j] and its sibling, ordered by
// bit l of the page; path[j][l] = the sibling. layer: the base tree's layer l
__global__ void __launch_bounds__(256) k_memtree_layer(const uint64_t *layer, const uint32_t *pg, const int32_t *prev,
                                                      size_t k, int l, int depth, const uint64_t *ver,
                                                      uint64_t *ver_next, uint64_t *paths) {
  const size_t t = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
  const int lane = threadIdx.x & 63, i = lane & 7;
  const size_t e = t >> 3;
  const bool ok = e < k;
  const size_t j = ok ? e : 0;
  const size_t node = (size_t)pg[j] >> l;
  const int32_t pv = prev[j * depth + l];
  const uint64_t own = ver[j * 4 + (i & 3)];
  const uint64_t sib = pv >= 0 ? ver[(size_t)pv * 4 + (i & 3)] : layer[(node ^ 1) * 4 + (i & 3)];
  if (ok && i < 4) paths[(j * depth + l) * 4 + i] = sib;
  uint64_t x = ((i < 4) == ((node & 1) == 0)) ? own : sib;
  x = permute8_lane(x, lane);
  if (ok && i < 4) ver_next[j * 4 + i] = x;
}

// the final version of every touched node goes into the base tree: exactly one op
// per (layer, node) has last set, so no two threads store to one word
struct LayerOffsets {
  size_t off[MEMTREE_MAX_DEPTH + 1];
};
__global__ void __launch_bounds__(256) k_memtree_writeback(uint64_t *nodes, LayerOffsets lo, const uint32_t *pg,
                                                          const uint8_t *last, size_t k, int depth,
                                                          const uint64_t *ver) {
  const size_t t = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
  const size_t w = t & 3, jl = t >> 2;
  if (jl >= k * (size_t)(depth + 1)) return;
  const size_t j = jl / (depth + 1), l = jl % (depth + 1);
  if (last[jl]) nodes[4 * (lo.off[l] + ((size_t)pg[j] >> l)) + w] = ver[(l * k + j) * 4 + w];
}

// ---------------------------------------------------------------- opening checks
// verify_memory_opening (commitments.rs:264-288) of ntask records, one 8-lane group
// each: the sponge of the record's row (k_merkle_leaves' for u64 words, k_memtree_leaves'
// for u32 words), folded with its `depth` siblings by the bits of its index, against its
// root -> ok[e] = 1 / 0. Task e reads row e and root e (root 0 when root_stride == 0);
// its index and path are record e's, or record e - span's for e >= span (ntask <= 2 span:
// the audit's second image of every record, under the same path). The index only
// orders the two children and is compared with nrows: it is never an address. Inputs
// come from outside, so every word is canonicalised. Groups past ntask run on a clamped
// record and store nothing; the sponge length and the depth are wave-uniform.
__device__ __forceinline__ uint64_t row_word(const uint64_t *row, size_t at) { return gl::canon(row[at]); }
__device__ __forceinline__ uint64_t row_word(const uint32_t *row, size_t at) { return row[at]; }

template <class Word>
__global__ void __launch_bounds__(256) k_merkle_verify(const Word *rows, size_t ntask, size_t span, size_t width,
                                                      size_t nrows, int depth, const uint32_t *index,
                                                      const uint64_t *paths, const uint64_t *roots,
                                                      size_t root_stride, uint8_t *ok) {
  const size_t t = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
  const int lane = threadIdx.x & 63, i = lane & 7;
  const size_t e = t >> 3;
  const bool live = e < ntask;
  const size_t j = live ? e : 0, rec = j >= span ? j - span : j;
  const Word *row = rows + j * width;
  uint64_t x = 0;
  for (size_t pos = 0; pos < width; pos += 4) {
    const size_t take = width - pos < 4 ? width - pos : 4;
    if ((size_t)i < take) x = row_word(row, pos + i);
    x = permute8_lane(x, lane);
  }
  const uint32_t idx = index[rec];
  uint32_t node = idx;
  const uint64_t *path = paths + rec * (size_t)depth * 4;
  for (int l = 0; l < depth; l++, node >>= 1) {
    const uint64_t own = shfl64(x, (lane & ~7) | (i & 3));  // the digest sits in the group's lanes 0..3
    const uint64_t sib = gl::canon(path[l * 4 + (i & 3)]);
    x = permute8_lane(((i < 4) == ((node & 1) == 0)) ? own : sib, lane);
  }
  int same = i >= 4 || x == gl::canon(roots[j * root_stride + (i & 3)]);
  same &= __shfl_xor(same, 1);
  same &= __shfl_xor(same, 2);
  if (live && i == 0) ok[e] = same && idx < nrows;
}

}  // namespace

int merkle_depth(size_t nrows) {
  size_t n = nrows <= 1 ? 1 : nrows + nrows % 2;
  int l = 0;
  for (; n > 1; l++) n = n == 2 ? 1 : ((n / 2 + 1) & ~(size_t)1);
  return l;
}

template <class Word>
hipError_t merkle_verify(const Word *rows, size_t ntask, size_t span, size_t width, size_t nrows,
                         const uint32_t *index, const uint64_t *paths, const uint64_t *roots, bool one_root,
                         uint8_t *ok, hipStream_t st) {
  if (!ntask) return hipSuccess;
  if (!nrows || !width || ntask > 2 * span || ntask > ((size_t)1 << 28)) return hipErrorInvalidValue;
  hipLaunchKernelGGL(k_merkle_verify<Word>, dim3(blocks(8 * ntask, 256)), dim3(256), 0, st, rows, ntask, span, width, nrows,
                     merkle_depth(nrows), index, paths, roots, one_root ? (size_t)0 : (size_t)4, ok);
  return hipGetLastError();
}
template hipError_t merkle_verify<uint64_t>(const uint64_t *, size_t, size_t, size_t, size_t, const uint32_t *,
                                            const uint64_t *, const uint64_t *, bool, uint8_t *, hipStream_t);
template hipError_t merkle_verify<uint32_t>(const uint32_t *, size_t, size_t, size_t, size_t, const uint32_t *,
                                            const uint64_t *, const uint64_t *, bool, uint8_t *, hipStream_t);

hipError_t p2w8_permute(uint64_t *states, size_t n, hipStream_t st) {
  if (!n) return hipSuccess;
  hipLaunchKernelGGL(k_p2w8_permute, dim3(blocks(n, 256)), dim3(256), 0, st, states, n);
  return hipGetLastError();
}

// Plonky3 MerkleTree::new over one matrix (p3-merkle-tree merkle_tree.rs at
// git 33e58c7787f9; not vendored): every layer but the root is padded to an even
// length with the zero digest (first_digest_layer: max_height + max_height % 2;
// compress: prev == 2 ? 1 : (prev / 2 + 1) & ~1), so any number of rows works
// (vm_code_comm, commitments.rs:314-340, commits a width-1 matrix of the code's
// half-words). nodes: the padded layers, leaves first, root last.
size_t merkle_nodes(size_t nrows) {
  size_t n = nrows <= 1 ? 1 : nrows + nrows % 2, tot = n;
  while (n > 1) {
    n = n == 2 ? 1 : ((n / 2 + 1) & ~(size_t)1);
    tot += n;
  }
  return tot;
}

hipError_t merkle_tree(const uint64_t *rows, size_t nrows, size_t width, uint64_t *nodes, hipStream_t st) {
  if (!nrows || !width) return hipErrorInvalidValue;
  hipLaunchKernelGGL(k_merkle_leaves, dim3(blocks(8 * nrows, 256)), dim3(256), 0, st, rows, nrows, width, nodes);
  size_t off = 0, n = nrows <= 1 ? 1 : nrows + nrows % 2;
  hipError_t e;
  if (n > nrows && (e = hipMemsetAsync(nodes + 4 * nrows, 0, 32 * (n - nrows), st)) != hipSuccess) return e;
  while (n > 1) {
    const size_t nn = n == 2 ? 1 : ((n / 2 + 1) & ~(size_t)1);
    hipLaunchKernelGGL(k_merkle_level, dim3(blocks(8 * (n / 2), 256)), dim3(256), 0, st, nodes + 4 * off, n / 2,
                       nodes + 4 * (off + n));
    if (nn > n / 2 && (e = hipMemsetAsync(nodes + 4 * (off + n + n / 2), 0, 32 * (nn - n / 2), st)) != hipSuccess)
      return e;
    off += n;
    n = nn;
  }
  return hipGetLastError();
}

// the first node of every padded layer, leaves first; the root's is the last entry
// (depth + 1 entries: merkle_nodes()'s recurrence)
int merkle_layer_offsets(size_t nrows, size_t *off, int max_layers) {
  size_t n = nrows <= 1 ? 1 : nrows + nrows % 2, at = 0;
  int l = 0;
  for (;; l++) {
    if (l >= max_layers) return -1;
    off[l] = at;
    if (n == 1) return l;
    at += n;
    n = n == 2 ? 1 : ((n / 2 + 1) & ~(size_t)1);
  }
}

hipError_t memtree_apply(uint64_t *nodes, size_t npages, size_t width, const MemtreeBatch &b, size_t k,
                         hipStream_t st) {
  if (!k) return hipSuccess;
  LayerOffsets lo;
  const int depth = merkle_layer_offsets(npages, lo.off, MEMTREE_MAX_DEPTH + 1);
  if (!npages || !width || depth < 0) return hipErrorInvalidValue;
  hipLaunchKernelGGL(k_memtree_leaves, dim3(blocks(8 * k, 256)), dim3(256), 0, st, b.pages, k, width, b.ver);
  for (int l = 0; l < depth; l++)
    hipLaunchKernelGGL(k_memtree_layer, dim3(blocks(8 * k, 256)), dim3(256), 0, st, nodes + 4 * lo.off[l], b.pg, b.prev, k, l,
                       depth, b.ver + (size_t)l * k * 4, b.ver + (size_t)(l + 1) * k * 4, b.paths);
  hipLaunchKernelGGL(k_memtree_writeback, dim3(blocks(4 * k * (depth + 1), 256)), dim3(256), 0, st, nodes, lo, b.pg, b.last, k,
                     depth, b.ver);
  return hipGetLastError();
}

// independent PaddingFreeSponge hashes of nrows rows (the leaf layer alone)
hipError_t hash_w8_rows(const uint64_t *rows, size_t nrows, size_t width, uint64_t *out, hipStream_t st) {
  if (!nrows) return hipSuccess;
  if (!width) return hipMemsetAsync(out, 0, 32 * nrows, st);  // the empty input's digest is the zero state
  hipLaunchKernelGGL(k_merkle_leaves, dim3(blocks(8 * nrows, 256)), dim3(256), 0, st, rows, nrows, width, out);
  return hipGetLastError();
}

}  // namespace lfk
