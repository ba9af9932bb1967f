// The chunked column pass ("The column pass").  A thread per column alone leaves the chip empty (10^4 columns = 40
// workgroups), so the rows are cut into chunks = min(COL_CHUNKS, rows) chunks of per = ceil(rows / chunks) consecutive rows
// (trailing chunks may be empty: rows = 33 uses 17 of its 32).  A pass kernel runs one thread per (chunk, column), walks its rows
// in ascending order and writes a partial to plane[chunk * cols + c] - an empty chunk its zero; a finishing kernel, one thread
// per column, adds the partials chunk 0 first.  No floating-point atomics: a result does not depend on scheduling, and every
// site agrees on the cut and the order, which is why replicates, surrogates and lanes reproduce to the bit.
#pragma once
#include "common.h"

namespace xmca {

constexpr int COL_CHUNKS = 32;
static inline int col_chunks(int64_t rows) { return (int)std::min<int64_t>(COL_CHUNKS, rows); }

struct ColChunk {            // what a pass functor is called with: column c, the rows [r0, r1) of `chunk`, at = chunk * cols + c
  int64_t c, at;
  int chunk, chunks, r0, r1;
};
__device__ inline ColChunk col_chunk(int64_t c, int64_t cols, int rows, int chunk, int chunks) {
  const int per = (rows + chunks - 1) / chunks;
  return {c, (int64_t)chunk * cols + c, chunk, chunks, chunk * per, min(rows, chunk * per + per)};
}

// The sum of the partials of column c, chunk 0 first.  It starts from zero: every partial accumulator starts at +0.0 (keep it
// so), hence a partial is never -0.0 and 0.0 + p == p for any other p - the same bits as a sum that starts from part[c].
template <typename V>
__device__ inline V chunk_sum(const V* __restrict__ part, int chunks, int64_t cols, int64_t c) {
  V s = 0;
#pragma unroll 8          // (the loads of a batch are issued together; the adds keep their order)
  for (int k = 0; k < chunks; ++k) s += part[(int64_t)k * cols + c];
  return s;
}

// f(ColChunk) for every (chunk, column), chunks = gridDim.y; f(c) for every column.  F: a small struct, passed by value.
template <typename F>
__global__ __launch_bounds__(256) void column_pass_kernel(int rows, int64_t cols, F f) {
  const int64_t c = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (c < cols) f(col_chunk(c, cols, rows, (int)blockIdx.y, (int)gridDim.y));
}
template <typename F>
__global__ __launch_bounds__(256) void column_finish_kernel(int64_t cols, F f) {
  const int64_t c = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (c < cols) f(c);
}

// The launches on the caller's stream; the planes inside `f` are the caller's and hold chunks * cols values each.
template <typename F>
static inline void column_pass(hipStream_t st, int rows, int64_t cols, int chunks, F f) {
  hipLaunchKernelGGL((column_pass_kernel<F>), dim3((unsigned)ceil_div(cols, 256), (unsigned)chunks), dim3(256), 0, st, rows, cols, f);
}
template <typename F>
static inline void column_finish(hipStream_t st, int64_t cols, F f) {
  hipLaunchKernelGGL((column_finish_kernel<F>), dim3((unsigned)ceil_div(cols, 256)), dim3(256), 0, st, cols, f);
}

}  // namespace xmca
