// tcsc_plan.h -- what the host-pointer API (tcsc_host.cpp) may use of the
// device-pointer API (tcsc_api.cpp), and nothing else: tcsc_gpu_plan stays an
// incomplete type here, so the host layer routes and sizes a call only through
// route_call() and never reads a plan's fields.  Not part of the public ABI.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "../../include/sparse/tcsc.h"
#include "../../include/tcsc_gpu.h"
#include "tcsc_internal.h"

// between two files of the library only: not in its dynamic symbol table
#pragma GCC visibility push(hidden)
namespace tcsc {

// ---- errors: the message behind tcsc_gpu_last_error() (set_error_msg() /
// error_msg() of tcsc_internal.h read and write the same thread's message)
void set_error(const char* fmt, ...);
int hip_fail(hipError_t e, const char* what);  // records the HIP error, returns TCSC_E_HIP

#define HIP_TRY(call)                                              \
    do {                                                           \
        hipError_t e_ = (call);                                    \
        if (e_ != hipSuccess) return ::tcsc::hip_fail(e_, #call);  \
    } while (0)

int device_count_raw();
int current_order();  // the summation order of plans created now (tcsc_gpu_set_order, $TCSC_ORDER)

class DeviceGuard {
  public:
    explicit DeviceGuard(int dev) {
        if (hipGetDevice(&prev_) != hipSuccess) prev_ = -1;
        ok_ = hipSetDevice(dev) == hipSuccess;
    }
    ~DeviceGuard() {
        if (prev_ >= 0) (void)hipSetDevice(prev_);
    }
    bool ok() const { return ok_; }

  private:
    int prev_ = -1;
    bool ok_ = false;
};

// ---- content fingerprint of a tcsc_t's index arrays (the host API's plan cache)
uint64_t fmix64(uint64_t h);
void hash_groups(const uint32_t* u, long long i0, long long i1, uint64_t acc[4]);
uint64_t hash_finish(const uint32_t* u, long long n, uint64_t h, uint64_t acc[4]);
uint64_t hash_ints(const int* p, long long n, uint64_t h);
uint64_t tcsc_fingerprint(const tcsc_t* W);

// tcsc_gpu_plan_create; allow_mfma false: never the MFMA image (the host API's exact mode)
int plan_create_impl(const tcsc_t* W, int col_begin, int col_end, int device, void* stream, bool allow_mfma,
                     tcsc_gpu_plan** out);

// ---- the route of one call ---------------------------------------------------
// Everything that launches, sizes or reports a call of M rows takes these from
// route_call(), which alone asks the cost models (use_decode / use_mfma /
// use_small, choose_slices, wide_pays, combine_mode).
struct Route {
    int path = TCSC_PATH_GATHER;
    // The K split as launched: the MFMA GEMM's, or the 16-column gather's
    // rounded to whole chunks (the grid's z).  The 22-column kernel runs
    // unsplit: the rounds model takes it only where this is 1, and where
    // $TCSC_GEO=22 forces it the queries still report the 16-column split and
    // its combine mode, as they always have.
    int slices = 1;
    int geo = 0;          // gather: kCW or kWideCW; -1 where $TCSC_GEO=22 cannot be had
    int combine = 0;      // gather: combine_mode of the split (0, 2, 3, 4)
    int rows = 0;         // gather: rows per launch, min(M, kMaxLaunchRows)
    size_t ws_bytes = 0;  // workspace the call needs; 0 where the plan cannot run a pinned path
};
// What the caller fixes.  A job cut into several launches (row bands, the
// 2^22-row pieces) pins the whole job's path and K split on every piece: the
// cost models are not monotone in M, and a piece on another path or split
// would sum in another order, in a workspace sized for the job's.
struct RoutePins {
    int path = TCSC_PATH_AUTO;  // AUTO: the cost models choose; GATHER can always be pinned, MFMA, SMALL and DECODE for sizing
    int slices = 0;             // > 0: the gather's K split (else $TCSC_SLICES, else the cost model)
    bool plan_ws = true;        // the launch runs on the plan's own workspace, beside its combine words
    bool vec = true;            // Y, B and the slabs are 16-B aligned and ldy % 4 == 0
};
constexpr size_t kUnbounded = (size_t)-1;  // ws_avail: size the call, whatever is reserved
// The route of a call of M rows of type dt (tcsc::kF32 / kBf16 / kI8) with
// ws_avail bytes of workspace to split K into.  A caller that launches or
// reports the geometry names itself in `who` and finds the message of a
// refused $TCSC_GEO=22 set.
Route route_call(const tcsc_gpu_plan* p, int M, int dt, size_t ws_avail, const RoutePins& pin,
                 const char* who = nullptr);

// What an entry point received: the one description of a call that travels
// from the public functions to the launch.  X is M x K of xtype (tcsc::kF32 /
// kBf16 / kI8; with the int8 type the row scales xscale, null for ones); y is
// the output (YOut, tcsc_internal.h): an fp32 or bf16 call's is {Y, kYF32,
// nullptr}, and the int8 call's decode and MFMA routes alone write anything
// else; ldy is in y's elements.  `who` is the name the call gives itself in
// messages (null: the activation type's own entry point).
// The up half of a gated call (tcsc_gpu_sgemm_i8_glu): the call's own plan, B and
// y.cscale are the gate's, Y = i8_glu(gate value, up value, act) in y's type.  G is the caller's
// scratch for the gate values of the MFMA route, M x ldg floats.  up == null: not a gated call.
struct GluUp {
    const tcsc_gpu_plan* up = nullptr;
    const float* cscale = nullptr;
    const float* B = nullptr;
    float* G = nullptr;
    int ldg = 0;
    int act = 0;
};
// The members beyond the first of a grouped call (tcsc_gpu_sgemm_i8_group): the call's own
// plan, B, y and ldy are member 0's, and every further member has a plan, bias, output (y.ytype the
// call's) and pitch of its own.  count == 0: not a grouped call.
struct GroupRest {
    struct Member {
        const tcsc_gpu_plan* plan = nullptr;
        const float* B = nullptr;
        YOut y;
        int ldy = 0;
    };
    int count = 0;
    Member m[kGroupMax - 1];
};
struct Call {
    const void* X = nullptr;
    int xtype = kF32;
    const float* xscale = nullptr;
    const float* B = nullptr;
    YOut y;
    int M = 0, ldy = 0, variant = 0;
    float a = 0.f;
    void* stream = nullptr;
    const char* who = nullptr;
    GluUp glu;
    GroupRest group;
    // The residual of a residual call (tcsc_gpu_sgemm_i8_res): M x ldr elements of y's
    // type, added to the call's value in the epilogue; it may be y.Y itself with ldr == ldy.  Null:
    // not a residual call.  Only the decode and MFMA routes of the int8 call serve one.
    const void* R = nullptr;
    int ldr = 0;
    // rows [r0, r0 + n) of a call on a matrix of K rows as a call of their own: X (x_elem bytes an
    // element), the row scales, Y and a residual call's R (by the element size of their type), a gated
    // call's G and every further member's Y of a grouped call advance by r0 rows
    Call rows(int r0, int n, int K, size_t x_elem) const {
        Call c = *this;
        c.X = X ? static_cast<const char*>(X) + (size_t)r0 * K * x_elem : nullptr;
        c.xscale = xscale ? xscale + r0 : nullptr;
        c.y = y.rows_on((size_t)r0, ldy);
        c.glu.G = glu.G ? glu.G + (size_t)r0 * glu.ldg : nullptr;
        c.R = R ? static_cast<const char*>(R) + (size_t)r0 * ldr * y.elem() : nullptr;
        for (int i = 0; i < group.count; ++i) c.group.m[i].y = group.m[i].y.rows_on((size_t)r0, group.m[i].ldy);
        c.M = n;
        return c;
    }
};
// a Call from an entry point's arguments, in the order the public prototypes list them
inline Call make_call(const void* X, int xtype, const float* xscale, const float* B, const YOut& y, int M, int ldy,
                      int variant, float a, void* stream, const char* who = nullptr) {
    Call c;
    c.X = X;
    c.xtype = xtype;
    c.xscale = xscale;
    c.B = B;
    c.y = y;
    c.M = M;
    c.ldy = ldy;
    c.variant = variant;
    c.a = a;
    c.stream = stream;
    c.who = who;
    return c;
}

// One call on a caller's workspace ws; the narrow types have stage 0 only.
// *ran, if given, receives the route that ran.
int sgemm_ws(const tcsc_gpu_plan* p, const Call& c, float* ws, size_t ws_bytes, int stage, const RoutePins& pin,
             Route* ran);

}  // namespace tcsc
#pragma GCC visibility pop
