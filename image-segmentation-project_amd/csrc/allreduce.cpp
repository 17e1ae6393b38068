// ---------------------------------------------------------------------------
// DDP gradient reduction over RCCL for non-Python hosts (SURVEY.md §8(b):
// "unet_allreduce_* ... communicator init from a ncclUniqueId byte blob";
// insertion point /root/reference/train.py:48-49).  RCCL is resolved at run
// time: the process's already-loaded RCCL (torch's, when a Python host loaded
// it globally) or /opt/rocm's librccl.so.1, so the library itself has no
// link-time RCCL dependency and plan-only / CPU users never load it.
// ---------------------------------------------------------------------------
#include <dlfcn.h>
#include <rccl/rccl.h>  // types only: the functions are resolved at run time (unet_allreduce_init)

#include <cstring>

#include "plan.h"

namespace {
struct Rccl {
  decltype(&ncclGetUniqueId) get_id = nullptr;
  decltype(&ncclCommInitRank) init = nullptr;
  decltype(&ncclCommDestroy) destroy = nullptr;
  decltype(&ncclAllReduce) allreduce = nullptr;
  decltype(&ncclGetErrorString) errstr = nullptr;
  bool ok = false;
};
const Rccl& rccl() {
  static Rccl r = [] {
    Rccl x;
    void* h = nullptr;
    if (!dlsym(RTLD_DEFAULT, "ncclCommInitRank")) {
      h = dlopen("librccl.so.1", RTLD_NOW | RTLD_LOCAL);
      if (!h) h = dlopen("/opt/rocm/lib/librccl.so.1", RTLD_NOW | RTLD_LOCAL);
    }
    auto sym = [&](const char* n) { return h ? dlsym(h, n) : dlsym(RTLD_DEFAULT, n); };
    x.get_id = reinterpret_cast<decltype(x.get_id)>(sym("ncclGetUniqueId"));
    x.init = reinterpret_cast<decltype(x.init)>(sym("ncclCommInitRank"));
    x.destroy = reinterpret_cast<decltype(x.destroy)>(sym("ncclCommDestroy"));
    x.allreduce = reinterpret_cast<decltype(x.allreduce)>(sym("ncclAllReduce"));
    x.errstr = reinterpret_cast<decltype(x.errstr)>(sym("ncclGetErrorString"));
    x.ok = x.get_id && x.init && x.destroy && x.allreduce && x.errstr;
    return x;
  }();
  return r;
}
int rccl_check(ncclResult_t r, const char* what) {
  if (r == ncclSuccess) return 0;
  set_err(std::string(what) + ": " + rccl().errstr(r));
  return 1;
}
}  // namespace

struct unet_comm {
  ncclComm_t comm = nullptr;
  int rank = 0, world = 1;
};

extern "C" {

static_assert(UNET_UNIQUE_ID_BYTES == NCCL_UNIQUE_ID_BYTES, "ncclUniqueId blob size");

int unet_allreduce_unique_id(void* id) {
  if (!id) { set_err("unet_allreduce_unique_id: null buffer"); return 1; }
  if (!rccl().ok) { set_err("unet_allreduce_unique_id: RCCL (librccl.so.1) not found"); return 1; }
  ncclUniqueId u;
  if (rccl_check(rccl().get_id(&u), "ncclGetUniqueId")) return 1;
  std::memcpy(id, &u, sizeof(u));
  return 0;
}

int unet_allreduce_init(const void* id, int rank, int world, unet_comm** out) {
  if (!id || !out || world < 1 || rank < 0 || rank >= world) {
    set_err("unet_allreduce_init: null argument or rank outside [0, world)");
    return 1;
  }
  if (!rccl().ok) { set_err("unet_allreduce_init: RCCL (librccl.so.1) not found"); return 1; }
  ncclUniqueId u;
  std::memcpy(&u, id, sizeof(u));
  unet_comm* c = new unet_comm();
  c->rank = rank;
  c->world = world;
  if (rccl_check(rccl().init(&c->comm, world, u, rank), "ncclCommInitRank")) {
    delete c;
    return 1;
  }
  *out = c;
  return 0;
}

void unet_allreduce_destroy(unet_comm* c) {
  if (!c) return;
  if (c->comm && rccl().ok) (void)rccl().destroy(c->comm);
  delete c;
}

int unet_allreduce_mean(unet_comm* c, float* buf, int64_t n, hipStream_t stream) {
  if (!c || n < 0 || (n > 0 && !buf)) { set_err("unet_allreduce_mean: null communicator / buffer"); return 1; }
  if (n == 0) return 0;
  return rccl_check(rccl().allreduce(buf, buf, (size_t)n, ncclFloat32, ncclAvg, c->comm, stream), "ncclAllReduce");
}

int unet_allreduce_bucket(unet_comm* c, unet_plan* p, float* grads, int bucket, hipStream_t comm_stream) {
  if (!c || !p || !grads || bucket < 0 || bucket >= (int)p->buckets.size()) {
    set_err("unet_allreduce_bucket: null argument or bad bucket");
    return 1;
  }
  // after the bucket's event when the last backward recorded one (DDP overlap);
  // otherwise the caller has ordered comm_stream after the whole backward
  if (bucket < p->nevents) CK(hipStreamWaitEvent(comm_stream, p->events[bucket], 0));
  const auto& r = p->buckets[(size_t)bucket];
  return unet_allreduce_mean(c, grads + r.first, r.second - r.first, comm_stream);
}

}  // extern "C"
