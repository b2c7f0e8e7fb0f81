// Device identity of split vGPUs on a real GPU (tests/test_gpu_vdev_identity.py): two host
// threads, T0 on HIP device 0 and T1 on device 1 - the two vGPUs of one GPU under the shim.
// Each reads who its device is (bus id, UUID, the properties' PCI fields), creates a stream,
// allocates 64 MiB with hipMalloc and 256 MiB with hipMallocAsync on its stream, stamps its
// hipMalloc buffer with one kernel on that stream and copies it back. T0 then asks for the
// device of T1's stream and of both of T1's pointers, at their base and inside them.
//
//   vdev_probe [--handshake]   -> one JSON line with what it saw; exit status 1 on any HIP error.
// With --handshake it prints {"phase": "before"} / {"phase": "after"} around T1's stream-ordered
// allocation (T0's follows) and waits for a line on its standard input each time, so that the
// caller can read the vGPUs' quota slots in between.
#include <hip/hip_runtime.h>

#include <condition_variable>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <mutex>
#include <thread>
#include <vector>

__global__ void stamp(uint32_t* p, size_t n, uint32_t v) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) p[i] = v;
}

namespace {

constexpr size_t kWords = 256 * 1024 + 3;  // no multiple of the block: the tail guard is exercised
constexpr size_t kMalloc = 64ull << 20, kAsync = 256ull << 20;

bool g_failed = false;
std::mutex g_fail_mu;

#define CHECK(x)                                                                  \
  do {                                                                            \
    hipError_t e_ = (x);                                                          \
    if (e_ != hipSuccess) {                                                       \
      fprintf(stderr, "%s failed: %s\n", #x, hipGetErrorString(e_));             \
      std::lock_guard<std::mutex> g_(g_fail_mu);                                  \
      g_failed = true;                                                            \
      return;                                                                     \
    }                                                                             \
  } while (0)

// A host thread that keeps its current device between the steps given to it.
class Worker {
 public:
  Worker() : th_([this] { loop(); }) {}
  ~Worker() {
    start(nullptr);
    th_.join();
  }
  void start(std::function<void()> f) {
    std::lock_guard<std::mutex> l(mu_);
    job_ = std::move(f);
    have_ = true;
    cv_.notify_all();
  }
  void wait() {
    std::unique_lock<std::mutex> l(mu_);
    cv_.wait(l, [&] { return !have_; });
  }

 private:
  void loop() {
    for (;;) {
      std::unique_lock<std::mutex> l(mu_);
      cv_.wait(l, [&] { return have_; });
      if (!job_) return;
      std::function<void()> f = job_;
      l.unlock();
      f();
      l.lock();
      have_ = false;
      cv_.notify_all();
    }
  }
  std::mutex mu_;
  std::condition_variable cv_;
  std::function<void()> job_;
  bool have_ = false;
  std::thread th_;
};

struct Tenant {
  int dev = 0;
  char bus[64] = {0};
  char uuid[33] = {0};
  int prop[3] = {-1, -1, -1};
  int by_bus = -1, stream_dev = -1, current = -1;
  hipStream_t stream = nullptr;
  char* buf = nullptr;    // hipMalloc
  char* abuf = nullptr;   // hipMallocAsync
  size_t bad = kWords;    // words that did not read back as dev + 1
};

void identify(Tenant* t) {
  CHECK(hipSetDevice(t->dev));
  CHECK(hipGetDevice(&t->current));
  CHECK(hipDeviceGetPCIBusId(t->bus, (int)sizeof(t->bus), t->dev));
  hipUUID u;
  CHECK(hipDeviceGetUuid(&u, t->dev));
  for (int i = 0; i < 16; i++) snprintf(t->uuid + 2 * i, 3, "%02x", (unsigned char)u.bytes[i]);
  hipDeviceProp_t p;
  CHECK(hipGetDeviceProperties(&p, t->dev));
  t->prop[0] = p.pciDomainID;
  t->prop[1] = p.pciBusID;
  t->prop[2] = p.pciDeviceID;
  CHECK(hipDeviceGetByPCIBusId(&t->by_bus, t->bus));
  CHECK(hipStreamCreate(&t->stream));
  CHECK(hipStreamGetDevice(t->stream, &t->stream_dev));
  CHECK(hipMalloc(reinterpret_cast<void**>(&t->buf), kMalloc));
}

void allocate_async(Tenant* t) {
  CHECK(hipMallocAsync(reinterpret_cast<void**>(&t->abuf), kAsync, t->stream));
  CHECK(hipStreamSynchronize(t->stream));
}

void stamp_and_check(Tenant* t) {
  static_assert(kWords * sizeof(uint32_t) <= kMalloc, "the stamped words lie inside the buffer");
  const unsigned block = 256, grid = (unsigned)((kWords + block - 1) / block);
  hipLaunchKernelGGL(stamp, dim3(grid), dim3(block), 0, t->stream, reinterpret_cast<uint32_t*>(t->buf), kWords,
                     (uint32_t)t->dev + 1);
  CHECK(hipGetLastError());
  std::vector<uint32_t> host(kWords, 0);
  CHECK(hipMemcpyAsync(host.data(), t->buf, kWords * sizeof(uint32_t), hipMemcpyDeviceToHost, t->stream));
  CHECK(hipStreamSynchronize(t->stream));
  size_t bad = 0;
  for (size_t i = 0; i < kWords; i++) bad += host[i] != (uint32_t)t->dev + 1;
  t->bad = bad;
}

void release(Tenant* t) {
  CHECK(hipFreeAsync(t->abuf, t->stream));
  CHECK(hipStreamSynchronize(t->stream));
  CHECK(hipFree(t->buf));
  CHECK(hipStreamDestroy(t->stream));
}

int pointer_device(const void* p) {
  int d = -1;
  if (hipPointerGetAttribute(&d, HIP_POINTER_ATTRIBUTE_DEVICE_ORDINAL, const_cast<void*>(p)) != hipSuccess) {
    std::lock_guard<std::mutex> g(g_fail_mu);
    g_failed = true;
    fprintf(stderr, "hipPointerGetAttribute(%p) failed\n", p);
  }
  return d;
}

struct Cross {
  int stream1 = -1, ptr1[2] = {-1, -1}, aptr1[2] = {-1, -1}, ptr0[2] = {-1, -1}, aptr0[2] = {-1, -1}, attrs1 = -1;
};

// On T0 (current device 0): the devices of T1's stream and pointers, and of T0's own.
void cross_query(const Tenant* t0, const Tenant* t1, Cross* c) {
  CHECK(hipStreamGetDevice(t1->stream, &c->stream1));
  c->ptr1[0] = pointer_device(t1->buf);
  c->ptr1[1] = pointer_device(t1->buf + kMalloc / 2 + 4);
  c->aptr1[0] = pointer_device(t1->abuf);
  c->aptr1[1] = pointer_device(t1->abuf + kAsync - 1);
  c->ptr0[0] = pointer_device(t0->buf);
  c->ptr0[1] = pointer_device(t0->buf + 1);
  c->aptr0[0] = pointer_device(t0->abuf);
  c->aptr0[1] = pointer_device(t0->abuf + kAsync / 2);
  hipPointerAttribute_t at;
  CHECK(hipPointerGetAttributes(&at, t1->buf + 4096));
  c->attrs1 = at.device;
}

void phase(bool handshake, const char* name) {
  if (!handshake) return;
  printf("{\"phase\": \"%s\"}\n", name);
  fflush(stdout);
  char line[16];
  if (!fgets(line, sizeof(line), stdin)) g_failed = true;  // the caller went away
}

template <typename F>
void both(Worker* w, Tenant* t, F f) {
  for (int i = 0; i < 2; i++) w[i].start([=] { f(&t[i]); });
  for (int i = 0; i < 2; i++) w[i].wait();
}

}  // namespace

int main(int argc, char** argv) {
  const bool handshake = argc > 1 && !strcmp(argv[1], "--handshake");
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess || n < 2) {
    fprintf(stderr, "vdev_probe needs two HIP devices (has %d)\n", n);
    return 1;
  }
  Tenant t[2];
  t[1].dev = 1;
  Cross c;
  {
    Worker w[2];
    both(w, t, identify);
    if (!g_failed) phase(handshake, "before");
    if (!g_failed) {  // T1 first, alone: the caller sees whose quota its 256 MiB went to
      w[1].start([&] { allocate_async(&t[1]); });
      w[1].wait();
    }
    if (!g_failed) phase(handshake, "after");
    if (!g_failed) {
      w[0].start([&] { allocate_async(&t[0]); });
      w[0].wait();
    }
    if (!g_failed) both(w, t, stamp_and_check);
    if (!g_failed) {
      w[0].start([&] { cross_query(&t[0], &t[1], &c); });
      w[0].wait();
    }
    if (!g_failed) both(w, t, release);
  }
  if (g_failed) return 1;
  printf("{\"words\": %zu, \"dev\": [", kWords);
  for (int i = 0; i < 2; i++)
    printf("%s{\"bus\": \"%s\", \"uuid\": \"%s\", \"prop\": [%d, %d, %d], \"by_bus\": %d, \"stream_dev\": %d, "
           "\"current\": %d, \"bad\": %zu}",
           i ? ", " : "", t[i].bus, t[i].uuid, t[i].prop[0], t[i].prop[1], t[i].prop[2], t[i].by_bus, t[i].stream_dev,
           t[i].current, t[i].bad);
  printf("], \"from_t0\": {\"stream1\": %d, \"ptr1\": [%d, %d], \"aptr1\": [%d, %d], \"ptr0\": [%d, %d], "
         "\"aptr0\": [%d, %d], \"attrs1\": %d}}\n",
         c.stream1, c.ptr1[0], c.ptr1[1], c.aptr1[0], c.aptr1[1], c.ptr0[0], c.ptr0[1], c.aptr0[0], c.aptr0[1], c.attrs1);
  return 0;
}
