// Which byte lands where in ds_read_b64_tr_b8 (gfx950): every lane of a 16-lane group addresses 8 bytes of LDS; the probe
// gives lane i of a group the bytes 8 i .. 8 i + 7 (and, in a second pass, its group's number) and prints what each lane gets.
// prefill_d256_fp8.hip addresses its V reads by the result: lane j of a group receives byte j of the eight 16-byte rows
// that lanes (2 r, 2 r + 1) address, r = 0 .. 7 - an [8][16] byte matrix transposed, inside each quarter wave.
// Build: hipcc -O3 --offload-arch=gfx950 tools/probes/ds_read_tr8.hip -o tools/ab/ds_read_tr8
#include <hip/hip_runtime.h>

#include <cstdio>

typedef __attribute__((ext_vector_type(2))) int i32x2;

__global__ __launch_bounds__(64) void probe(unsigned char* out) {
  __shared__ __attribute__((aligned(16))) unsigned char lds[1024];
  const int lane = threadIdx.x;
  for (int pass = 0; pass < 2; ++pass) {
    for (int i = lane; i < 512; i += 64) lds[i] = pass == 0 ? (unsigned char)(i & 127) : (unsigned char)(i >> 7);
    __syncthreads();
    const i32x2 v = __builtin_amdgcn_ds_read_tr8_b64_v2i32((__attribute__((address_space(3))) i32x2*)(lds + 8 * lane));
    *(i32x2*)(out + pass * 512 + 8 * lane) = v;
    __syncthreads();
  }
}

int main() {
  unsigned char *d, h[1024];
  if (hipMalloc(&d, 1024) != hipSuccess) return 1;
  hipLaunchKernelGGL(probe, dim3(1), dim3(64), 0, 0, d);
  if (hipMemcpy(h, d, 1024, hipMemcpyDeviceToHost) != hipSuccess) return 1;
  bool transposed = true;
  for (int lane = 0; lane < 64; ++lane) {
    printf("lane %2d:", lane);
    for (int b = 0; b < 8; ++b) {
      printf(" %3d", h[8 * lane + b]);
      transposed = transposed && h[8 * lane + b] == 16 * b + (lane & 15) && h[512 + 8 * lane + b] == (lane >> 4);
    }
    printf("   group %d\n", h[512 + 8 * lane]);
  }
  printf("[8][16] transpose inside each quarter wave: %s\n", transposed ? "yes" : "NO");
  return 0;
}
