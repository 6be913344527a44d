// tlagen_sort.hip — the one library kernel the generated path needs that is not generated: the
// radix sort of a level's winner keys in TLC's FIFO order (tlagen_kernels.h, pass 1 -> pass 2).
// The generated code object (hiprtc) holds the spec's kernels; the sort is spec independent.
#include <hip/hip_runtime.h>

#include <rocprim/device/device_radix_sort.hpp>

namespace rmc {

// keys_in[0, n) -> keys_out ascending over the low `bits` bits, with the caller's temporary buffer of
// *tmp_bytes; tmp == nullptr: nothing is sorted, *tmp_bytes = the temporary bytes this sort needs
int tlagen_sort_keys(const unsigned long long* keys_in, unsigned long long* keys_out, unsigned long long n, int bits,
                     void* tmp, size_t* tmp_bytes, hipStream_t s) {
  size_t have = *tmp_bytes;
  if (rocprim::radix_sort_keys(tmp, have, keys_in, keys_out, (size_t)n, 0, bits, s) != hipSuccess) return -1;
  if (!tmp) *tmp_bytes = have;
  return 0;
}

// ---- checkpoint writer (tlagen_backend.cpp save_checkpoint): the stored states in id order.
// The search appends a level's states to the store in the order its lanes reach the word counter,
// so the same states lie differently from run to run; a checkpoint holds them packed in id order
// (ckpt_file.h GenHead), which TLC's FIFO order makes the same bytes every time.

// sizes[i] = words of state first + i: the lengths in its nv variables' headers (0: a header that
// runs past the stored words, which the writer refuses)
__global__ void __launch_bounds__(256) tlagen_sizes_k(const unsigned int* words, unsigned long long used, const unsigned long long* offs,
                                                      unsigned long long first, unsigned long long n, int nv, unsigned long long* sizes) {
  for (unsigned long long i = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (unsigned long long)gridDim.x * blockDim.x) {
    const unsigned long long q0 = offs[first + i];
    unsigned long long q = q0;
    bool ok = true;
    for (int v = 0; v < nv && ok; ++v) {
      const unsigned long long len = q < used ? (unsigned long long)(words[q] >> 3) : 0ull;
      ok = len != 0 && len <= used - q;
      q += len;
    }
    sizes[i] = ok ? q - q0 : 0ull;
  }
}

// out[at[i] .. at[i + 1]) = the words of state first + i (a wave per state; at[n] closes the last)
__global__ void __launch_bounds__(256) tlagen_pack_k(const unsigned int* words, const unsigned long long* offs, unsigned long long first,
                                                     unsigned long long n, const unsigned long long* at, unsigned int* out) {
  const unsigned long long wave = ((unsigned long long)blockIdx.x * blockDim.x + threadIdx.x) / 64, waves = (unsigned long long)gridDim.x * blockDim.x / 64;
  const unsigned int lane = threadIdx.x % 64;
  for (unsigned long long i = wave; i < n; i += waves) {
    const unsigned int* src = words + offs[first + i];
    const unsigned long long o = at[i], len = at[i + 1] - o;
    for (unsigned long long q = lane; q < len; q += 64) out[o + q] = src[q];
  }
}

int tlagen_state_sizes(const unsigned int* words, unsigned long long used, const unsigned long long* offs, unsigned long long first,
                       unsigned long long n, int nv, unsigned long long* sizes, hipStream_t s) {
  if (!n) return 0;
  const unsigned blocks = (unsigned)std::min<unsigned long long>(4096, (n + 255) / 256);
  hipLaunchKernelGGL(tlagen_sizes_k, dim3(blocks), dim3(256), 0, s, words, used, offs, first, n, nv, sizes);
  return hipGetLastError() == hipSuccess ? 0 : -1;
}
int tlagen_pack_states(const unsigned int* words, const unsigned long long* offs, unsigned long long first, unsigned long long n,
                       const unsigned long long* at, unsigned int* out, hipStream_t s) {
  if (!n) return 0;
  const unsigned blocks = (unsigned)std::min<unsigned long long>(8192, (n + 3) / 4);
  hipLaunchKernelGGL(tlagen_pack_k, dim3(blocks), dim3(256), 0, s, words, offs, first, n, at, out);
  return hipGetLastError() == hipSuccess ? 0 : -1;
}

}  // namespace rmc
