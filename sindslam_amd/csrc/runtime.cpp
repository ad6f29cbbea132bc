// What the whole library owns: the process set-up at load time, the thread-local error string (sind_set_error / sind_last_error), the wait counters and the
// roctx marker loader.
#include <cstdarg>
#include "common.hpp"

// ---------------------------------------------------------------- process set-up
// HIP streams are multiplexed onto GPU_MAX_HW_QUEUES hardware queues (runtime default 4).  A pipeline handle drives ~45 streams; with four queues its flow slices share queues
// with the tail streams and a stand-alone sequence job runs 17 % slower, six keep them apart, ten and more are catastrophic (profiles/r04/hw_queues.txt).  The runtime reads
// the variable when it initialises (the first HIP call of the process), so the library sets it when it is LOADED -- for the C++ integrator who links libsind_hip.so as much
// as for the Python mirror.  An explicit setting in the environment wins; a process whose HIP runtime is already up keeps what it started with.
__attribute__((constructor)) static void sind_process_setup() { setenv("GPU_MAX_HW_QUEUES", "6", 0); }

// ---------------------------------------------------------------- error string (shared by the whole library)
static thread_local char g_err[512] = "";
std::atomic<long long> g_sind_wait_ns{0}, g_sind_wait_calls{0};
thread_local SindHostGate* t_sind_gate = nullptr;
thread_local int t_sind_spin_us = 0;

#include <dlfcn.h>
#include <cstring>
#include <cstdlib>
namespace {
struct Roctx { int (*push)(const char*) = nullptr; int (*pop)() = nullptr;
    // The marker library is only looked for when a profiler is attached (rocprofv3 preloads librocprofiler-sdk-tool / sets ROCP_TOOL_LIBRARIES) or SIND_ROCTX=1
    // asks for it: a production process does not dlopen profiler libraries.
    static bool wanted() {
        if (const char* e = getenv("SIND_ROCTX")) return atoi(e) != 0;
        for (const char* v : {"ROCP_TOOL_LIBRARIES", "ROCPROFILER_REGISTER_FORCE_LOAD", "ROCPROF_OUTPUT_PATH"}) if (getenv(v)) return true;
        const char* pre = getenv("LD_PRELOAD"); return pre && strstr(pre, "rocprofiler");
    }
    Roctx() {
        if (!wanted()) return;
        for (const char* lib : {"librocprofiler-sdk-roctx.so.1", "librocprofiler-sdk-roctx.so", "libroctx64.so.4", "libroctx64.so"}) {
            if (void* so = dlopen(lib, RTLD_NOW | RTLD_LOCAL)) {
                push = (int (*)(const char*))dlsym(so, "roctxRangePushA"); pop = (int (*)())dlsym(so, "roctxRangePop");
                if (push && pop) return;
                push = nullptr; pop = nullptr; (void)dlclose(so);
            }
        }
    } };
Roctx& roctx() { static Roctx r; return r; }
}  // namespace
void sind_range_push(const char* name) { if (roctx().push) (void)roctx().push(name); }
void sind_range_pop() { if (roctx().pop) (void)roctx().pop(); }
void sind_set_error(const char* fmt, ...) { va_list ap; va_start(ap, fmt); vsnprintf(g_err, sizeof(g_err), fmt, ap); va_end(ap); }
extern "C" const char* sind_last_error() { return g_err; }
