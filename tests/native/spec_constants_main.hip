// spec_constants_main.hip -- the device expressions the value image of the compiled kernels replaces (csrc/odw_build.h:
// spec_image_build), evaluated on the GPU as intersect_prim (csrc/odw_kernels.hip) writes them for the generic kernels.
//
//   spec_constants_main in.bin out.bin
//
// in.bin: records of 6 doubles (primitive kind, its 4 parameters, distTol); out.bin: 4 doubles per record, the constants
// in the image's order (unused ones 0).  tests/test_gpu_spec_image.py compiles this file with the options the compiled
// kernels get (-O3 -ffp-contract=on: a product and a sum of one expression fuse, nothing else does) and holds the output
// against the image bit for bit.
#include <hip/hip_runtime.h>

#include <cstdio>
#include <vector>

#include "../../include/odw_trace.h"

__global__ void constants_kernel(const double* __restrict__ in, double* __restrict__ out, int n) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const double* par = in + 6 * (size_t)i + 1;
  const int type = (int)in[6 * (size_t)i];
  const double tol = in[6 * (size_t)i + 5];
  double* o = out + 4 * (size_t)i;
  o[0] = o[1] = o[2] = o[3] = 0.0;
  if (type == ODW_PRIM_BOX) {
    o[0] = par[0] + tol;
    o[1] = par[1] + tol;
    o[2] = par[2] + tol;
  } else if (type == ODW_PRIM_TORUS) {
    const double R1 = par[0], R2 = par[1];
    const double bound = (R1 + R2) * 1.0000001 + 1e-9;
    const double zs = R2 * 1.0000001 + 1e-9;
    const double rin = (R1 - R2) * 0.9999999 - 1e-9;
    o[0] = bound;
    o[1] = zs;
    o[2] = rin;
    o[3] = rin * rin;
  } else if (type == ODW_PRIM_CYLINDER || type == ODW_PRIM_CONE || type == ODW_PRIM_PARABOLOID) {
    const bool parab = type == ODW_PRIM_PARABOLOID;
    const double R1 = parab ? 0.0 : par[0];
    const double R2 = (type == ODW_PRIM_CYLINDER) ? par[0] : (parab ? par[2] : par[1]);
    const double H = (type == ODW_PRIM_CONE) ? par[2] : par[1];
    o[0] = H + tol;
    const double lim = R1 * R1 * (1.0 - 1e-9);
    o[1] = lim;
    o[2] = (R1 + tol) * (R1 + tol);
    o[3] = (R2 + tol) * (R2 + tol);
  }
}

#define CHECK(call)                                                                      \
  do {                                                                                   \
    hipError_t e_ = (call);                                                              \
    if (e_ != hipSuccess) { std::printf("%s: %s\n", #call, hipGetErrorString(e_)); return 2; } \
  } while (0)

int main(int argc, char** argv) {
  if (argc != 3) { std::printf("usage: %s in.bin out.bin\n", argv[0]); return 1; }
  FILE* f = std::fopen(argv[1], "rb");
  if (!f) { std::printf("cannot read %s\n", argv[1]); return 1; }
  std::fseek(f, 0, SEEK_END);
  const long bytes = std::ftell(f);
  std::fseek(f, 0, SEEK_SET);
  const int n = (int)(bytes / (6 * sizeof(double)));
  std::vector<double> in((size_t)n * 6), out((size_t)n * 4);
  if (n < 1 || std::fread(in.data(), sizeof(double), in.size(), f) != in.size()) { std::fclose(f); std::printf("short file\n"); return 1; }
  std::fclose(f);
  double *d_in = nullptr, *d_out = nullptr;
  CHECK(hipMalloc(&d_in, in.size() * sizeof(double)));
  CHECK(hipMalloc(&d_out, out.size() * sizeof(double)));
  CHECK(hipMemcpy(d_in, in.data(), in.size() * sizeof(double), hipMemcpyHostToDevice));
  hipLaunchKernelGGL(constants_kernel, dim3((n + 255) / 256), dim3(256), 0, 0, d_in, d_out, n);
  CHECK(hipGetLastError());
  CHECK(hipMemcpy(out.data(), d_out, out.size() * sizeof(double), hipMemcpyDeviceToHost));
  CHECK(hipFree(d_in));
  CHECK(hipFree(d_out));
  f = std::fopen(argv[2], "wb");
  if (!f || std::fwrite(out.data(), sizeof(double), out.size(), f) != out.size()) { std::printf("cannot write %s\n", argv[2]); return 1; }
  std::fclose(f);
  std::printf("%d records\n", n);
  return 0;
}
