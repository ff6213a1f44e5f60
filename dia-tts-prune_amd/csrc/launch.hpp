// One launch path for every kernel of the library.  Normally a plain hipLaunchKernelGGL.  While a recorder is armed
// (dia_engine_time_step, dia_gemm_timed) each launch is bracketed by its own dispatch-level start / stop events
// (hipExtLaunchKernelGGL): the timestamps come from the dispatch packet itself — kernel begin / end, the quantity
// rocprofv3 --kernel-trace reports — not from markers between launches.
//
// Dynamic LDS above 64 KiB needs the kernel's MaxDynamicSharedMemorySize attribute raised first, for that exact
// instantiation.  dia_launch does it: each instantiation remembers the largest limit raised for it so far, and a launch
// that asks for more raises it to its own smem.  A failed raise skips the launch; the caller's dia_check_launch reports
// it, and a later launch tries again.  The limit applies to the current device.
#pragma once
#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>
#include <atomic>
#include <mutex>
#include <vector>
#include <utility>

struct dia_launch_recorder {
  bool armed = false;
  std::vector<std::pair<hipEvent_t, hipEvent_t>> ev;
  std::vector<const void*> fn;          // host function of every recorded launch (resolved to its name at collect time)
};
dia_launch_recorder& dia_recorder();          // thread-local
// arm: subsequent launches of this thread are recorded.  collect: synchronises on the last stop event, writes the
// kernel durations (ms, launch order) into out[0..cap) and, when asked, the end-to-end intervals between consecutive
// kernels, returns their count (or a negative DIA_E_*), disarms and releases the events.
void dia_recorder_arm();
int dia_recorder_collect(float* out_ms, int cap, float* out_interval_ms = nullptr);
// kernel instantiation name of the i-th launch of the last collected recording ("k_gemv_small<8, 8, 2, false>"), or ""
const char* dia_recorder_label(int i);
// this thread's launch was skipped because its dynamic-LDS limit could not be raised: the next dia_check_launch(kernel)
// returns DIA_E_HIP with a message naming the attribute call and the kernel
void dia_note_lds_raise_failed(hipError_t e);

// raises kern's dynamic-LDS limit to smem unless `raised` already covers it.  One lock for all kernels: two threads
// cannot leave the smaller of their values in force.
inline bool dia_raise_lds(const void* kern, size_t smem, std::atomic<size_t>& raised) {
  static std::mutex mu;
  std::lock_guard<std::mutex> lock(mu);
  if (smem <= raised.load(std::memory_order_relaxed)) return true;
  const hipError_t e = hipFuncSetAttribute(kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem);
  if (e != hipSuccess) { dia_note_lds_raise_failed(e); return false; }
  raised.store(smem, std::memory_order_release);
  return true;
}

template <auto Kern, typename... Args>
inline void dia_launch(dim3 grid, dim3 block, size_t smem, hipStream_t st, Args... args) {
  static std::atomic<size_t> raised{64 * 1024};     // dynamic-LDS limit in force for this instantiation
  if (smem > raised.load(std::memory_order_acquire) && !dia_raise_lds(reinterpret_cast<const void*>(Kern), smem, raised)) return;
  dia_launch_recorder& r = dia_recorder();
  if (r.armed) {
    hipEvent_t e0 = nullptr, e1 = nullptr;
    (void)hipEventCreate(&e0); (void)hipEventCreate(&e1);
    hipExtLaunchKernelGGL(Kern, grid, block, smem, st, e0, e1, 0, args...);
    r.ev.emplace_back(e0, e1);
    r.fn.push_back(reinterpret_cast<const void*>(Kern));
  } else {
    hipLaunchKernelGGL(Kern, grid, block, smem, st, args...);
  }
}
