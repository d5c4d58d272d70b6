// Device helpers; see device.hpp.
#include "mireduce/device.hpp"

#include <atomic>

namespace mireduce {

DeviceInfo device_info(int dev) {
  hipDeviceProp_t p;
  MIREDUCE_HIP_THROW(hipGetDeviceProperties(&p, dev));
  DeviceInfo d;
  d.id = dev;
  d.name = p.name;
  d.arch = p.gcnArchName;
  d.cus = p.multiProcessorCount;
  d.total_mem = p.totalGlobalMem;
  d.clock_khz = p.clockRate;
  return d;
}

int device_count() {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) return 0;
  return n;
}

int device_cus(int device) {
  static std::atomic<int> cached[64];  // 0: not asked yet (racing first calls store the same value)
  if (device < 0) MIREDUCE_HIP_THROW(hipGetDevice(&device));
  std::atomic<int>* const slot = device < 64 ? &cached[device] : nullptr;
  int cus = slot ? slot->load(std::memory_order_relaxed) : 0;
  if (cus > 0) return cus;
  MIREDUCE_HIP_THROW(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device));
  if (cus <= 0) cus = 256;
  if (slot) slot->store(cus, std::memory_order_relaxed);
  return cus;
}

EventTimer::EventTimer() {
  MIREDUCE_HIP_THROW(hipEventCreate(&a_));
  MIREDUCE_HIP_THROW(hipEventCreate(&b_));
}

EventTimer::~EventTimer() {
  if (a_) (void)hipEventDestroy(a_);
  if (b_) (void)hipEventDestroy(b_);
}

void EventTimer::start(hipStream_t s) { MIREDUCE_HIP_THROW(hipEventRecord(a_, s)); }
void EventTimer::stop(hipStream_t s) { MIREDUCE_HIP_THROW(hipEventRecord(b_, s)); }

float EventTimer::elapsed_ms() {
  MIREDUCE_HIP_THROW(hipEventSynchronize(b_));
  float ms = 0;
  MIREDUCE_HIP_THROW(hipEventElapsedTime(&ms, a_, b_));
  return ms;
}

void DeviceBuffer::allocate(size_t bytes) {
  release();
  if (bytes) MIREDUCE_HIP_THROW(hipMalloc(&p_, bytes));
  n_ = bytes;
}

void DeviceBuffer::release() {
  if (p_) (void)hipFree(p_);
  p_ = nullptr;
  n_ = 0;
}

}  // namespace mireduce
