// Shared host-side helpers of liblbdrn_hip: error string, HIP call checking, geometry helpers.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>

#include <atomic>

#include "../../include/lbdrn_hip.h"

namespace lbdrn {

void set_error(const char* fmt, ...);   // error_buffer.inc: one buffer per shared library
const char* last_error();

#define LBDRN_HIP_TRY(expr)                                                                  \
    do {                                                                                     \
        hipError_t e_ = (expr);                                                              \
        if (e_ != hipSuccess) {                                                              \
            ::lbdrn::set_error("%s failed: %s (%s:%d)", #expr, hipGetErrorString(e_), __FILE__, \
                               __LINE__);                                                    \
            return LBDRN_E_DEVICE;                                                           \
        }                                                                                    \
    } while (0)

#define LBDRN_REQUIRE(cond, ...)            \
    do {                                    \
        if (!(cond)) {                      \
            ::lbdrn::set_error(__VA_ARGS__); \
            return LBDRN_E_ARG;             \
        }                                   \
    } while (0)

// kernels are launched with <<<>>>; this turns a launch failure into a status
#define LBDRN_LAUNCH_CHECK() LBDRN_HIP_TRY(hipGetLastError())

inline int64_t param_count(const lbdrn_net& n)
{
    int64_t c = 0;
    for (int l = 0; l < n.nl; ++l) c += (int64_t)n.bc * (l ? n.bc : n.F) + n.bc;
    return c + (int64_t)n.C * n.bc + n.C;
}
// offset of layer l's weight matrix in the flat parameter vector (l == nl: last layer)
inline int64_t layer_offset(const lbdrn_net& n, int l)
{
    int64_t c = 0;
    for (int i = 0; i < l; ++i) c += (int64_t)n.bc * (i ? n.bc : n.F) + n.bc;
    return c;
}
inline int feature_dim(const lbdrn_geom& g)
{
    const int side = 2 * g.D + 1;
    return 2 * g.P + (g.use_colors ? g.C * side * side : 0);
}
inline size_t align_up(size_t x, size_t a) { return (x + a - 1) / a * a; }
// The geometry the launches of an entry point read: the caller's, with the divisor of the normalisation at least 1.  An
// MSB plane that is zero everywhere (msb_max == 0: every sample below 2^K) would make every colour feature 0 / 0; it is
// normalised by 1, so its features are exact zeros (lbdrn_hip.h, at msb_max).  Nothing changes for msb_max >= 1.
inline lbdrn_geom launch_geom(const lbdrn_geom& g)
{
    lbdrn_geom r = g;
    if (r.msb_max < 1) r.msb_max = 1;
    return r;
}

// the dynamic-LDS ceiling of a kernel is told to the runtime once per device and kernel (a cache of an idempotent
// setting; several host threads may get here together)
template <class K>
static int configure_lds_once(K kern, int bytes, std::atomic<unsigned long long>& configured)
{
    int dev = 0;
    (void)hipGetDevice(&dev);
    const unsigned long long bit = 1ull << (dev & 63);
    if (!(configured.load(std::memory_order_relaxed) & bit)) {
        LBDRN_HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, bytes));
        configured.fetch_or(bit, std::memory_order_relaxed);
    }
    return 0;
}

int check_geom(const lbdrn_geom* g);
int check_net(const lbdrn_net* n);

// ---- generic path (generic.hip)
int generic_split_bits(const uint16_t* img, int C, int H, int W, int K, uint16_t* msb, int32_t* mx,
                       hipStream_t s);
int generic_labels(const uint16_t* img, int C, int H, int W, int K, const int64_t* idx, int64_t n,
                   float* labels, hipStream_t s);
int generic_features(const lbdrn_geom& g, const uint16_t* msb, const int64_t* idx, int64_t n,
                     int64_t first, float* out, hipStream_t s);
size_t generic_forward_workspace(const lbdrn_net& net, int64_t B);
int generic_forward(const lbdrn_net& net, const float* params, const float* x, int64_t B, float* y,
                    void* ws, size_t ws_bytes, hipStream_t s);
size_t generic_apply_workspace(const lbdrn_geom& g, const lbdrn_net& net);
int generic_decode(const lbdrn_geom& g, const lbdrn_net& net, const uint16_t* msb,
                   const float* params, uint16_t* out, float* y_out, void* ws, size_t ws_bytes,
                   hipStream_t s);
int generic_eval_sse(const lbdrn_geom& g, const lbdrn_net& net, const uint16_t* img,
                     const uint16_t* msb, const float* params, double* sse, void* ws,
                     size_t ws_bytes, int nodata, bool decoded, hipStream_t s);   // nodata: LBDRN_EVAL_VALID's sample value, or -1; decoded: LBDRN_EVAL_DECODED
size_t generic_train_workspace(const lbdrn_net& net, int B);
int generic_train_step(const lbdrn_net& net, const float* x, const float* t, int B, float* params,
                       float* m, float* v, int64_t adam_step, double lr, int apply_adam,
                       float* loss, float* grads, void* ws, size_t ws_bytes, hipStream_t s);
size_t generic_tape_bytes(const lbdrn_net& net, int64_t B);
size_t generic_backward_workspace(const lbdrn_net& net, int64_t B);
int generic_forward_tape(const lbdrn_net& net, const float* params, const float* x, int64_t B, float* y, void* tape,
                         size_t tape_bytes, hipStream_t s);
int generic_backward(const lbdrn_net& net, const float* params, const float* x, int64_t B, const void* tape,
                     size_t tape_bytes, const float* y, const float* dy, float* grads, float* dx, void* ws,
                     size_t ws_bytes, hipStream_t s);
int generic_train_epoch(const lbdrn_geom& g, const lbdrn_net& net, const uint16_t* img,
                        const uint16_t* msb, const int64_t* perm, int64_t n, int bs, float* params,
                        float* m, float* v, int64_t step0, double lr, float* losses, void* ws,
                        size_t ws_bytes, hipStream_t s);

// ---- fused MFMA path (apply_mfma.hip)
bool mfma_apply_supported(const lbdrn_geom& g, const lbdrn_net& net);
size_t mfma_apply_workspace(const lbdrn_geom& g, const lbdrn_net& net);
int mfma_decode(const lbdrn_geom& g, const lbdrn_net& net, const uint16_t* msb, const float* params,
                uint16_t* out, float* y_out, void* ws, size_t ws_bytes, hipStream_t s);
int mfma_eval_sse(const lbdrn_geom& g, const lbdrn_net& net, const uint16_t* img,
                  const uint16_t* msb, const float* params, double* sse, void* ws, size_t ws_bytes,
                  bool background, bool fast, bool x16, int nodata, bool decoded, hipStream_t s);   // decoded: LBDRN_EVAL_DECODED, never with fast
// whether the instance that serves this evaluation request reads msb (host arithmetic; false: it takes img >> K)
bool mfma_eval_reads_msb(const lbdrn_geom& g, const lbdrn_net& net, bool fast, bool x16);
// which instance serves a request (0 decode, 1 evaluation, 2 fast, 3 exact-operand) and on what plan: lbdrn_apply_instance's out[8]
bool mfma_apply_instance(const lbdrn_geom& g, const lbdrn_net& net, int request, int32_t out[8]);

int mfma_train_epoch_group(int count, const lbdrn_geom& g, const lbdrn_net& net, const int64_t* const* perm, int64_t n,
                           int bs, float* const* params, float* const* m, float* const* v, int64_t step0, double lr,
                           float* const* losses, void* const* ws, size_t ws_bytes, hipStream_t s, bool alone);

}  // namespace lbdrn
