/*
 * A HIP runtime that launches nothing: the handful of entry points libgpd.so's HOST code calls, for the host-side sanitizer build
 * (tests/test_host_sanitizers.py: the five units -- step_rollout.hip, policy.hip, swarm.hip, abi.hip, mrac.hip -- compiled
 * `--cuda-host-only -fsanitize=address,undefined`, linked against this file instead of libamdhip64).  Kernel launches are counted, their
 * geometry recorded and their kernel NAMED (the handle a launch passes is the one the unit registered its device symbol under), so the
 * test can also hold the launch arithmetic (grid and block sizes, dynamic LDS) and the choice of the kernel against what a call should
 * get -- on a machine without a GPU.  Test infrastructure.
 */
#include <stddef.h>
#include <stdlib.h>
#include <string.h>

typedef struct { unsigned x, y, z; } dim3_;
static __thread dim3_ t_grid, t_block;
static __thread size_t t_shmem;
static __thread void* t_stream;
static int g_launches;
static unsigned g_last[7];          /* grid xyz | block xyz | dynamic LDS bytes */
static struct Kernel { const void* host_fn; const char* dev_name; }* g_kernels;     /* every registered kernel (grows as needed) */
static size_t g_kernel_count, g_kernel_cap;
static const char* g_last_kernel = "?";
static void (*g_on_launch)(const char* kernel, const unsigned geometry[7]);

int __hipPushCallConfiguration(dim3_ grid, dim3_ block, size_t shmem, void* stream) {
    t_grid = grid; t_block = block; t_shmem = shmem; t_stream = stream;
    return 0;
}
int __hipPopCallConfiguration(dim3_* grid, dim3_* block, size_t* shmem, void** stream) {
    *grid = t_grid; *block = t_block; *shmem = t_shmem; *stream = t_stream;
    return 0;
}
void** __hipRegisterFatBinary(const void* data) { static void* handle; (void)data; return &handle; }
void __hipRegisterFunction(void** modules, const void* host_fn, char* dev_fn, const char* dev_name, unsigned limit, void* tid, void* bid,
                           void* bdim, void* gdim, int* wsize) {
    (void)modules; (void)dev_fn; (void)limit; (void)tid; (void)bid; (void)bdim; (void)gdim; (void)wsize;
    if (g_kernel_count == g_kernel_cap) {
        g_kernel_cap = g_kernel_cap ? 2 * g_kernel_cap : 256;
        g_kernels = realloc(g_kernels, g_kernel_cap * sizeof *g_kernels);
        if (!g_kernels) abort();
    }
    g_kernels[g_kernel_count].host_fn = host_fn;
    g_kernels[g_kernel_count++].dev_name = dev_name;      /* (a string of the registering library: it outlives the table) */
}
void __hipRegisterVar(void** modules, void* var, char* host_name, char* dev_name, int ext, size_t size, int constant, int global) {
    (void)modules; (void)var; (void)host_name; (void)dev_name; (void)ext; (void)size; (void)constant; (void)global;
}
void __hipUnregisterFatBinary(void** modules) { (void)modules; }

int hipLaunchKernel(const void* fn, dim3_ grid, dim3_ block, void** args, size_t shmem, void* stream) {
    (void)args; (void)stream;
    ++g_launches;
    g_last_kernel = "?";
    for (size_t i = 0; i < g_kernel_count; ++i)
        if (g_kernels[i].host_fn == fn) { g_last_kernel = g_kernels[i].dev_name; break; }
    g_last[0] = grid.x; g_last[1] = grid.y; g_last[2] = grid.z; g_last[3] = block.x; g_last[4] = block.y; g_last[5] = block.z;
    g_last[6] = (unsigned)shmem;
    if (g_on_launch) g_on_launch(g_last_kernel, g_last);
    return 0;
}
int hipGetLastError(void) { return 0; }
const char* hipGetErrorString(int e) { return e ? "stub error" : "no error"; }
int hipGetDevice(int* dev) { *dev = 0; return 0; }
int hipDeviceGetAttribute(int* value, int attr, int dev) { (void)attr; (void)dev; *value = 100000; return 0; }
int hipMalloc(void** p, size_t n) { *p = calloc(1, n ? n : 1); return *p ? 0 : 2; }
int hipFree(void* p) { free(p); return 0; }
int hipHostMalloc(void** p, size_t n, unsigned flags) { (void)flags; *p = calloc(1, n ? n : 1); return *p ? 0 : 2; }
int hipMemcpyAsync(void* dst, const void* src, size_t n, int kind, void* stream) { (void)kind; (void)stream; memcpy(dst, src, n); return 0; }
int hipStreamSynchronize(void* stream) { (void)stream; return 0; }
int hipMemcpyFromSymbolAsync(void* dst, const void* sym, size_t n, size_t off, int kind, void* stream) {
    (void)sym; (void)off; (void)kind; (void)stream; memset(dst, 0, n); return 0;
}
int hipMemcpyToSymbolAsync(const void* sym, const void* src, size_t n, size_t off, int kind, void* stream) {
    (void)sym; (void)src; (void)n; (void)off; (void)kind; (void)stream; return 0;
}

/* what the test reads */
int hipstub_launches(void) { return g_launches; }
void hipstub_last(unsigned out[7]) { memcpy(out, g_last, sizeof g_last); }
void hipstub_on_launch(void (*f)(const char*, const unsigned[7])) { g_on_launch = f; }     /* called at every launch (NULL: nobody) */
const char* hipstub_last_kernel(void) { return g_last_kernel; }      /* the device symbol of the last launch, "?" for an unknown handle */
