// C ABI of the plan handle (include/unet_hip.h): creation and introspection,
// the forward / backward entries, timing, profiling and bucket events.
#include <cstdio>
#include <exception>

#include "plan.h"

thread_local std::string unet::g_err;

#define API_GUARD(body)                                    \
  try {                                                    \
    body                                                   \
  } catch (const std::exception& e) {                      \
    set_err(std::string("exception: ") + e.what());        \
    return 1;                                              \
  } catch (...) {                                          \
    set_err("unknown exception");                          \
    return 1;                                              \
  }

extern "C" {

const char* unet_last_error(void) { return g_err.c_str(); }
const char* unet_version(void) { return "unet_hip 0.1 gfx950"; }

int unet_plan_create(const unet_config* cfg, unet_plan** out) {
  API_GUARD({
    if (!cfg || !out) { set_err("null argument"); return 1; }
    unet_plan* p = new unet_plan();
    p->cfg = *cfg;
    const int r = build_plan(p);
    if (r) { delete p; return r; }
    *out = p;
    return 0;
  })
}

void unet_plan_destroy(unet_plan* p) {
  if (!p) return;
  if (p->tim_buf) (void)hipFree(p->tim_buf);
  for (int i = 0; i < p->nevents; ++i) (void)hipEventDestroy(p->events[i]);
  delete p;
}

int64_t unet_plan_workspace_bytes(const unet_plan* p) { return p ? (int64_t)p->ws_bytes : -1; }
int unet_plan_num_params(const unet_plan* p) { return p ? (int)p->params.size() : -1; }
int unet_plan_param_name(const unet_plan* p, int i, char* buf, int buflen) {
  if (!p || i < 0 || i >= (int)p->params.size() || !buf || buflen <= 0) { set_err("bad index"); return 1; }
  std::snprintf(buf, (size_t)buflen, "%s", p->params[i].name.c_str());
  return 0;
}
int unet_plan_param_shape(const unet_plan* p, int i, int64_t shape[4]) {
  if (!p || i < 0 || i >= (int)p->params.size()) { set_err("bad index"); return -1; }
  const auto& s = p->params[i].shape;
  for (size_t k = 0; k < s.size() && k < 4; ++k) shape[k] = s[k];
  return (int)s.size();
}
int64_t unet_plan_param_offset(const unet_plan* p, int i) {
  if (!p || i < 0 || i >= (int)p->params.size()) return -1;
  return p->params[i].flat;
}
int64_t unet_plan_grad_numel(const unet_plan* p) { return p ? p->grad_numel : -1; }
int unet_plan_num_bn(const unet_plan* p) { return p ? (int)p->bns.size() : -1; }
int unet_plan_num_buckets(const unet_plan* p) { return p ? (int)p->buckets.size() : -1; }
int unet_plan_bucket_range(const unet_plan* p, int b, int64_t* begin, int64_t* end) {
  if (!p || b < 0 || b >= (int)p->buckets.size()) { set_err("bad bucket"); return 1; }
  *begin = p->buckets[b].first;
  *end = p->buckets[b].second;
  return 0;
}
double unet_plan_flops(const unet_plan* p, int training) {
  return p ? (training ? p->flops_train : p->flops_fwd) : -1.0;
}

int unet_plan_num_tensors(const unet_plan* p) { return p ? (int)p->named.size() : -1; }
int unet_plan_tensor_info(const unet_plan* p, int i, char* name, int namelen, int64_t info[5]) {
  if (!p || i < 0 || i >= (int)p->named.size() || !name || namelen <= 0) { set_err("bad tensor index"); return 1; }
  const auto& t = p->named[i];
  std::snprintf(name, (size_t)namelen, "%s", t.first.c_str());
  info[0] = (int64_t)t.second.off; info[1] = t.second.ld; info[2] = t.second.C;
  info[3] = t.second.H; info[4] = t.second.W;
  return 0;
}

int unet_forward(unet_plan* p, const float* image, const float* const* params, float* const* buffers,
                 void* workspace, float* logits, int training, hipStream_t stream) {
  API_GUARD({
    if (!p || !image || !params || !buffers || !workspace || !logits) { set_err("null argument"); return 1; }
    const int r = run_forward(p, image, params, buffers, reinterpret_cast<char*>(workspace), logits, training, stream);
    if (r == 0 && p->f8n) p->f8_calibrated = true;
    return r;
  })
}

int unet_backward(unet_plan* p, const float* image, const float* dlogits, const float* const* params,
                  void* workspace, float* grads, hipStream_t stream) {
  API_GUARD({
    if (!p || !image || !dlogits || !params || !workspace || !grads) { set_err("null argument"); return 1; }
    return run_backward(p, image, dlogits, params, reinterpret_cast<char*>(workspace), grads, stream);
  })
}

int unet_set_conv_config(int cfg) {
  set_conv_config(cfg);
  return 0;
}

int unet_plan_use_bucket_events(unet_plan* p, int on) {
  if (!p) { set_err("null plan"); return 1; }
  p->want_events = on != 0;
  return 0;
}

int unet_timing_enable(unet_plan* p, int on) {
  if (!p) { set_err("null plan"); return 1; }
  const size_t bytes = (size_t)kTimLaunches * kTimBlocks * kTimSlots * sizeof(unsigned long long);
  if (on && !p->tim_buf) CK(hipMalloc(&p->tim_buf, bytes));
  if (on) CK(hipMemset(p->tim_buf, 0, bytes));
  p->tim_on = on != 0;
  p->tim_n = 0;
  p->tim_names.clear();
  return 0;
}

int64_t unet_timing_read(unet_plan* p, unsigned long long* host, int64_t max_launches, char* names, int64_t nlen) {
  if (!p || !p->tim_buf) { set_err("timing not enabled"); return -1; }
  CK(hipDeviceSynchronize());
  const int64_t n = p->tim_n < max_launches ? p->tim_n : max_launches;
  if (host && n > 0)
    CK(hipMemcpy(host, p->tim_buf, (size_t)n * kTimBlocks * kTimSlots * sizeof(unsigned long long),
                 hipMemcpyDeviceToHost));
  std::string all;
  for (int64_t i = 0; i < n; ++i) all += p->tim_names[(size_t)i] + "\n";
  if (names && nlen > 0) std::snprintf(names, (size_t)nlen, "%s", all.c_str());
  return n;
}

int unet_profile_enable(unet_plan* p, int on) {
  if (!p) { set_err("null plan"); return 1; }
  p->prof = on != 0;
  p->recs.clear();
  p->evused = 0;
  return 0;
}

int unet_profile_report(unet_plan* p, char* buf, int64_t buflen) {
  if (!p) { set_err("null plan"); return -1; }
  std::string out;
  if (!p->recs.empty()) {
    if (hipEventSynchronize(p->evpool[p->recs.back().e1]) != hipSuccess) { set_err("event sync failed"); return -1; }
  }
  char num[64];
  for (const auto& r : p->recs) {
    float ms = 0.f;
    if (hipEventElapsedTime(&ms, p->evpool[r.e0], p->evpool[r.e1]) != hipSuccess) ms = -1.f;
    // names of batched launches list every layer: no fixed-size line buffer
    std::snprintf(num, sizeof(num), "\t%.6f\t%.6e\t", ms, r.flops);
    out += r.name;
    out += num;
    out += r.kernel;
    out += '\n';
  }
  if (buf && buflen > 0) std::snprintf(buf, (size_t)buflen, "%s", out.c_str());
  return (int)out.size() + 1;
}

int unet_bucket_wait(unet_plan* p, int bucket, hipStream_t waiter) {
  if (!p || bucket < 0 || bucket >= p->nevents) { set_err("bad bucket"); return 1; }
  CK(hipStreamWaitEvent(waiter, p->events[bucket], 0));
  return 0;
}

}  // extern "C"
