// CPU only: the HIP calls the Monotonic entry points of one build of libgnf_hip.so make, as text two builds can be diffed on.
//
//   hipcc -x c++ -D__HIP_PLATFORM_AMD__ -I$ROCM_PATH/include -rdynamic tools/mono_launch_trace.cpp -o mono_launch_trace -ldl
//   ./mono_launch_trace path/to/libgnf_hip.so > trace.txt      (GNF_MONO_INDW / GNF_MONO_INV_PTS / GNF_TRUE_F32 as wanted)
//
// The program defines the few HIP runtime symbols a launch goes through (fat-binary registration, the <<< >>> call
// configuration, hipLaunchKernel, hipFuncSetAttribute, hipMemsetAsync, hipGetLastError) and exports them, so the library
// binds to these instead of the runtime's: no GPU is touched, every device pointer is a made-up address that nothing reads.
// One line per call: kernel name, grid, block, dynamic LDS bytes; attribute and memset calls with their sizes; then the entry
// point's return code.  Kernel ARGUMENTS are not printed (they hold the made-up addresses).
#include <hip/hip_runtime_api.h>
#include <dlfcn.h>
#include <cstdio>
#include <cstdlib>
#include <map>
#include <string>
#include <vector>
#include "../include/gnf_hip.h"

static std::map<const void*, std::string> g_names;
static dim3 g_grid, g_block;
static size_t g_shmem;
static hipStream_t g_stream;
static const char* name_of(const void* f) { return g_names.count(f) ? g_names[f].c_str() : "?"; }

extern "C" {
void** __hipRegisterFatBinary(const void*) { static void* h; return &h; }
void __hipUnregisterFatBinary(void**) {}
void __hipRegisterFunction(void**, const void* host, char*, const char* dev, unsigned, void*, void*, void*, void*, int*) { g_names[host] = dev; }
void __hipRegisterVar(void**, void*, char*, char*, int, size_t, int, int) {}
void __hipRegisterManagedVar(void*, void**, void*, const char*, size_t, unsigned) {}
hipError_t __hipPushCallConfiguration(dim3 g, dim3 b, size_t sh, hipStream_t s) { g_grid = g; g_block = b; g_shmem = sh; g_stream = s; return hipSuccess; }
hipError_t __hipPopCallConfiguration(dim3* g, dim3* b, size_t* sh, hipStream_t* s) { *g = g_grid; *b = g_block; *sh = g_shmem; *s = g_stream; return hipSuccess; }
hipError_t hipLaunchKernel(const void* f, dim3 g, dim3 b, void**, size_t sh, hipStream_t) {
  printf("  launch %s grid %u block %u lds %zu\n", name_of(f), g.x, b.x, sh);
  return hipSuccess;
}
hipError_t hipFuncSetAttribute(const void* f, hipFuncAttribute at, int v) { printf("  attr %s %d = %d\n", name_of(f), (int)at, v); return hipSuccess; }
hipError_t hipMemsetAsync(void*, int v, size_t n, hipStream_t) { printf("  memset %d x %zu\n", v, n); return hipSuccess; }
hipError_t hipGetLastError(void) { return hipSuccess; }
}

template <class F>
static F sym(void* lib, const char* n) {
  void* p = dlsym(lib, n);
  if (!p) { fprintf(stderr, "missing %s\n", n); exit(2); }
  return (F)p;
}

int main(int argc, char** argv) {
  void* lib = dlopen(argv[1], RTLD_NOW);
  if (!lib) { fprintf(stderr, "%s\n", dlerror()); return 2; }
  auto fwd = sym<decltype(&gnf_monotonic_fwd)>(lib, "gnf_monotonic_fwd"), fwd32 = sym<decltype(&gnf_monotonic_fwd)>(lib, "gnf_monotonic_fwd_f32");
  auto bwd = sym<decltype(&gnf_monotonic_bwd)>(lib, "gnf_monotonic_bwd"), bwd32 = sym<decltype(&gnf_monotonic_bwd)>(lib, "gnf_monotonic_bwd_f32");
  auto inv = sym<decltype(&gnf_monotonic_inv)>(lib, "gnf_monotonic_inv");
  auto wsb = sym<decltype(&gnf_monotonic_bwd_ws_bytes)>(lib, "gnf_monotonic_bwd_ws_bytes");
  auto fk = sym<decltype(&gnf_monotonic_fwd_kernel)>(lib, "gnf_monotonic_fwd_kernel"), bk = sym<decltype(&gnf_monotonic_bwd_kernel)>(lib, "gnf_monotonic_bwd_kernel");
  float* P = (float*)0x10000000;         // made-up device addresses, 16-byte aligned, never read
  std::vector<std::vector<int>> nets;
  for (int H : {1, 10, 16, 17, 32, 33, 48, 49, 50, 51, 52, 64, 65, 97, 100, 112, 113, 145, 150, 160, 161, 200, 256})
    for (int NH = 1; NH <= 5; ++NH) nets.push_back(std::vector<int>(NH, H));
  for (auto m : std::vector<std::vector<int>>{{40, 64, 24}, {97, 110, 101}, {145, 158, 147}, {100, 150, 100}, {48, 50, 50, 50}}) nets.push_back(m);
  const int64_t ns[] = {1, 40, 63, 301, 512, 513, 700, 4097, 8193, 9000, 78400};
  for (auto& hid : nets)
    for (int c : {5, 30, 33, 600}) {
      gnf_mono_net net{};
      net.nl = (int)hid.size() + 1;
      net.dims[0] = 1 + c;
      for (size_t i = 0; i < hid.size(); ++i) net.dims[i + 1] = hid[i];
      net.dims[net.nl] = 1;
      std::string tag;
      for (int h : hid) tag += std::to_string(h) + "-";
      float* gW[GNF_MONO_MAX_LAYERS]; float* gb[GNF_MONO_MAX_LAYERS];
      for (int l = 0; l < GNF_MONO_MAX_LAYERS; ++l) gW[l] = gb[l] = P;
      for (int64_t n : ns)
        for (int S : {5, 7, 20, 27, 31, 32, 40}) {
          if (n > 9000 && S != 20) continue;      // the large size at S = 20 only
          printf("%sc%d n%lld S%d\n", tag.c_str(), c, (long long)n, S);
          {
            const int64_t d = n > 100 && n % 7 == 0 ? 7 : 1, B = n / d;
            printf(" fwd -> %d", fwd(P, &net, P, P, d * c, c, 1, P, P, S, P, P, B, d, nullptr)); printf(" [%s]\n", fk());
            printf(" fwd_f32 -> %d", fwd32(P, &net, P, P, d * c, c, 1, P, P, S, P, P, B, d, nullptr)); printf(" [%s]\n", fk());
            printf(" inv -> %d\n", inv(P, &net, P, P, d * c, c, 1, P, P, S, P, B, d, nullptr));
            const int64_t full = wsb(&net, S, B, d), one = wsb(&net, S, 1, 1);
            for (int64_t ws : {full, one, (int64_t)64})      // whole, chunks of 16 elements, too small (GNF_EWS)
              for (auto f : {bwd, bwd32}) {
                if (ws == one && n > 700) continue;
                printf(" %s ws %lld -> %d", f == bwd ? "bwd" : "bwd_f32", (long long)ws,
                       f(P, &net, P, P, d * c, c, 1, P, P, S, P, P, P, P, d * c, c, 1, gW, gb, P, ws, B, d, nullptr));
                printf(" [%s]\n", bk());
              }
          }
        }
    }
  return 0;
}
