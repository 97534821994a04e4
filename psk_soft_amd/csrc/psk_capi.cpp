// psk_capi.cpp -- the C ABI of libpsk_soft_hip.so (include/psk_soft_hip.h).
//
// Host side of the drop-in boundary: per-channel control plane (psk_ctl.h, mirrors the
// non-data state of psk_soft_i, reference cpp/psk_soft.cpp:353-426), HBM-resident channel
// state, plan upload and kernel launches.  There is no CPU compute path here: without a
// usable GPU psk_soft_create() fails (PSK_SOFT_ERR_NO_DEVICE) unless the caller explicitly
// asks for a control-plane-only handle (PSK_SOFT_DEVICE_NONE), which never touches data.
#include <hip/hip_runtime_api.h>
#include <hip/hip_vector_types.h>

#include <atomic>
#include <cmath>
#include <condition_variable>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <memory>
#include <mutex>
#include <new>
#include <string>
#include <thread>
#include <vector>

#include "psk_acquire.h"
#include "psk_symrate.h"
#include "psk_sync.h"
#include "psk_demap.h"
#include "psk_viterbi.h"
#include "psk_rs.h"
#include "psk_frame.h"
#include "psk_ctl.h"
#include "psk_gather.h"
#include "psk_plan.h"
#include "psk_quality.h"
#include "psk_soft_hip.h"
#include "psk_fir.h"
#include "psk_resample.h"
#include "psk_tune.h"

namespace psk {
hipError_t launch_fast(int S, int H, int exact, const ChanPlan *plans, const uint32_t *list, uint32_t ch0, uint32_t nch, ChanState *states,
                       float2 *rings, uint32_t ring_cap, float *yvs, uint32_t fit_cap, uint32_t y_len, uint32_t r_len,
                       hipStream_t stream);
hipError_t launch_seq(const ChanPlan *plans, const uint32_t *list, uint32_t ch0, uint32_t nch, ChanState *states, float2 *rings,
                      uint32_t ring_cap, float *yvs, uint32_t fit_cap, hipStream_t stream);
hipError_t launch_read_probe(const void *src, uint64_t bytes, float *sink, hipStream_t stream);
// complex int16, complex int8 and complex binary16 packets (psk_pkt.hip; fmt: the PSK_SOFT_FORMAT_* value): the conversion pre-pass
hipError_t launch_convert(int fmt, const CvtDesc *desc, uint32_t n_desc, uint64_t max_n, hipStream_t stream);
// ... and the wave-scan and reference-order kernels that read them in place (psk_fast_inst.hip / psk_kernels.hip built with
// PSK_INST_PKT): numAvg <= 128, samplesPerBaud 2 .. 16, screened and exact tier
bool fast_pkt_has(int fmt, int S);
hipError_t launch_fast_pkt(int fmt, int S, int exact, const ChanPlan *plans, const uint32_t *list, uint32_t ch0, uint32_t nch, ChanState *states,
                           float2 *rings, uint32_t ring_cap, float *yvs, uint32_t fit_cap, uint32_t y_len, uint32_t r_len, hipStream_t stream);
hipError_t launch_seq_pkt(int fmt, const ChanPlan *plans, const uint32_t *list, uint32_t ch0, uint32_t nch, ChanState *states, float2 *rings,
                          uint32_t ring_cap, float *yvs, uint32_t fit_cap, hipStream_t stream);
// time-tiled kernels (psk_tile.hip)
bool tile_front_has(int S, int H);
hipError_t launch_tile_front(int S, int H, const ChanPlan *plans, const uint32_t *list, uint32_t ch0, uint32_t nch, uint32_t max_tiles,
                             const ChanState *states, const float2 *rings, uint32_t ring_cap, uint32_t r_len, TileInfo *tiles, float *t_raw,
                             float2 *t_s, PfChan *pf_chan, uint32_t tile0, hipStream_t stream);
hipError_t launch_tile_front_any(const ChanPlan *plans, const uint32_t *list, uint32_t ch0, uint32_t nch, uint32_t max_tiles, uint32_t max_S,
                                 const ChanState *states, const float2 *rings, uint32_t ring_cap, TileInfo *tiles, float *t_raw, float2 *t_s,
                                 PfChan *pf_chan, hipStream_t stream);
hipError_t launch_tile_fit(const ChanPlan *plans, const uint32_t *list, uint32_t ch0, uint32_t nch, ChanState *states, float2 *rings,
                           uint32_t ring_cap, float *yvs, uint32_t fit_cap, uint32_t y_len, TileInfo *tiles, const float *t_raw,
                           const float2 *t_s, float *t_est, const PfScratch &sc, hipStream_t stream);
// wide symbols, samplesPerBaud > kSeqMaxS: the front stage of the time-tiled kernels (psk_wide.hip) and the reference-order kernel
// with symbolEnergy[] in device memory (psk_kernels.hip built with PSK_SEQ_WIDE=1)
hipError_t launch_wide_front(const ChanPlan *plans, const uint32_t *list, uint32_t ch0, uint32_t nch, uint32_t max_tiles, uint32_t max_S,
                             const float2 *rings, uint32_t ring_cap, TileInfo *tiles, float *t_raw, float2 *t_s, PfChan *pf_chan, void *rec,
                             void *wst, hipStream_t stream);
size_t wide_rec_bytes();
size_t wide_stat_bytes();
uint32_t wide_chunks(uint32_t S);
hipError_t launch_seq_wide(const void *plans, const uint32_t *list, uint32_t ch0, uint32_t nch, void *states, float2 *rings,
                           uint32_t ring_cap, float *yvs, uint32_t fit_cap, double *symE, uint32_t symE_stride, hipStream_t stream);
hipError_t launch_pfit(const ChanPlan *plans, const uint32_t *list, uint32_t ch0, uint32_t nch, uint32_t max_tiles, ChanState *states,
                       float2 *rings, uint32_t ring_cap, float *yvs, uint32_t fit_cap, uint32_t y_len, TileInfo *tiles, const float *t_raw,
                       const float2 *t_s, float *t_est, const PfScratch &sc, bool second_round, hipStream_t stream);
hipError_t launch_tile_fit_range(const ChanPlan *plans, const uint32_t *list, uint32_t ch0, uint32_t nch, ChanState *states, float2 *rings,
                                 uint32_t ring_cap, float *yvs, uint32_t fit_cap, uint32_t y_len, TileInfo *tiles, const float *t_raw,
                                 const float2 *t_s, float *t_est, void *carry, float *carry_y, uint32_t tile0, uint32_t ntiles,
                                 hipStream_t stream);
size_t pipe_carry_bytes();
// PSK_SOFT_OPT_FAR_FIT (psk_farfit.hip): the fit stage for phaseAvg above kFastFitMax, its rings in rows of a scratch in device memory
hipError_t launch_far_fit(const ChanPlan *plans, const uint32_t *list, uint32_t ch0, uint32_t nch, ChanState *states, float2 *rings,
                          uint32_t ring_cap, float *yvs, uint32_t fit_cap, float *far_y, uint32_t far_rows, TileInfo *tiles,
                          const float *t_raw, const float2 *t_s, float *t_est, hipStream_t stream);
hipError_t launch_far_quiet(const ChanPlan *plans, const uint32_t *list, uint32_t ch0, uint32_t nch, ChanState *states, float2 *rings,
                            uint32_t ring_cap, float *yvs, uint32_t fit_cap, float *far_y, uint32_t far_rows, hipStream_t stream);
size_t far_ring_bytes();
hipError_t launch_tile_back(const ChanPlan *plans, const uint32_t *list, uint32_t ch0, uint32_t nch, uint32_t max_tiles,
                            const ChanState *states, const TileInfo *tiles, const float2 *t_s, const float *t_est, uint32_t tile0,
                            uint32_t early, hipStream_t stream);
}  // namespace psk

namespace {

thread_local std::string g_last_error;  // (psk_soft_last_error)

psk_soft_status fail(psk_soft_status st, const std::string &msg)
{
    g_last_error = msg;
    return st;
}

#define PSK_HIP(call)                                                                             \
    do {                                                                                          \
        hipError_t e_ = (call);                                                                   \
        if (e_ != hipSuccess)                                                                     \
            return fail(PSK_SOFT_ERR_HIP, std::string(#call) + ": " + hipGetErrorString(e_));     \
    } while (0)
// (a step that fails ends the function with its status, the message as the step left it)
#define PSK_TRY(call)                       \
    do {                                    \
        const psk_soft_status s_ = (call);  \
        if (s_ != PSK_SOFT_OK)              \
            return s_;                      \
    } while (0)

// n and a quarter more: what a buffer that is grown on demand is given when n no longer fit
inline size_t with_headroom(size_t n) { return n + n / 4u + 256u; }

// ---- ownership ("Ownership") ----
// Whatever the handle holds of the HIP runtime -- device memory, pinned memory, events, streams -- is a member of one of the four
// types below, in the handle or in a struct the handle contains: the destructor gives it back, and nothing else does.  None can be
// copied.  An empty owner makes no HIP call, in any method or in its destructor: a control-plane-only handle never touches the runtime.
struct DeviceMem {
    static hipError_t alloc(void **p, size_t bytes) { return hipMalloc(p, bytes); }
    static void free(void *p) { (void)hipFree(p); }
};
struct PinnedMem {
    static hipError_t alloc(void **p, size_t bytes) { return hipHostMalloc(p, bytes); }
    static void free(void *p) { (void)hipHostFree(p); }
};
// memory of either kind, in bytes (what grow_scratch sees of a buffer) ...
template <class Mem>
class OwnedBytes {
public:
    OwnedBytes() = default;
    OwnedBytes(const OwnedBytes &) = delete;
    OwnedBytes &operator=(const OwnedBytes &) = delete;
    ~OwnedBytes() { release(); }
    void release()
    {
        if (p_)
            Mem::free(p_);
        p_ = nullptr;
    }
    // what is held is released, then `bytes` are allocated; a failure leaves the owner empty
    hipError_t alloc_bytes(size_t bytes)
    {
        release();
        const hipError_t e = Mem::alloc(&p_, bytes);
        if (e != hipSuccess)
            p_ = nullptr;
        return e;
    }

protected:
    void *p_ = nullptr;
};
// ... and as n elements of T; reads as the T * it holds
template <class T, class Mem>
class OwnedBuf : public OwnedBytes<Mem> {
public:
    hipError_t alloc(size_t n) { return this->alloc_bytes(sizeof(T) * n); }
    T *get() const { return static_cast<T *>(this->p_); }
    operator T *() const { return get(); }
};
template <class T>
using DeviceBuf = OwnedBuf<T, DeviceMem>;
template <class T>
using PinnedBuf = OwnedBuf<T, PinnedMem>;

// An event (no timing, unless asked for) and whether it has been recorded since it was last cleared: both waits do nothing on one
// that was not.  Created by ensure() where its site creates it, else by its first record.
class Event {
public:
    Event() = default;
    Event(const Event &) = delete;
    Event &operator=(const Event &) = delete;
    ~Event()
    {
        if (ev_)  // (what it stands behind may be on a stream the caller brought, which nobody else waits for)
            (void)sync(), (void)hipEventDestroy(ev_);
    }
    explicit operator bool() const { return ev_ != nullptr; }
    hipEvent_t get() const { return ev_; }
    hipError_t ensure(bool timing = false)
    {
        if (ev_)
            return hipSuccess;
        return timing ? hipEventCreate(&ev_) : hipEventCreateWithFlags(&ev_, hipEventDisableTiming);
    }
    hipError_t record(hipStream_t stream)
    {
        if (const hipError_t e = ensure())
            return e;
        const hipError_t e = hipEventRecord(ev_, stream);
        recorded_ = recorded_ || e == hipSuccess;
        return e;
    }
    bool recorded() const { return recorded_; }
    void clear() { recorded_ = false; }  // (it has completed, or what it stood for is void: nothing waits for it again)
    hipError_t wait(hipStream_t stream) const { return recorded_ ? hipStreamWaitEvent(stream, ev_, 0) : hipSuccess; }  // `stream` waits
    hipError_t sync() const { return recorded_ ? hipEventSynchronize(ev_) : hipSuccess; }                              // the host waits

private:
    hipEvent_t ev_ = nullptr;
    bool recorded_ = false;
};

// A non-blocking stream, created where its site creates it; the destructor waits for what it carries.
class Stream {
public:
    Stream() = default;
    Stream(const Stream &) = delete;
    Stream &operator=(const Stream &) = delete;
    ~Stream()
    {
        if (s_)
            (void)hipStreamSynchronize(s_), (void)hipStreamDestroy(s_);
    }
    hipError_t create() { return hipStreamCreateWithFlags(&s_, hipStreamNonBlocking); }
    hipError_t create(int priority) { return hipStreamCreateWithPriority(&s_, hipStreamNonBlocking, priority); }
    hipError_t sync() const { return s_ ? hipStreamSynchronize(s_) : hipSuccess; }
    operator hipStream_t() const { return s_; }

private:
    hipStream_t s_ = nullptr;
};

// Device memory of n zeroed T in `out`, `what` in the message of a failure.  The memset is through before a launch on any stream
// reads or writes the memory.
template <class T>
psk_soft_status alloc_zeroed(DeviceBuf<T> &out, size_t n, const char *what)
{
    PSK_HIP(out.alloc(n));
    if (hipMemset(out, 0, sizeof(T) * n) != hipSuccess || hipDeviceSynchronize() != hipSuccess) {
        out.release();
        return fail(PSK_SOFT_ERR_HIP, std::string(what) + ": hipMemset failed");
    }
    return PSK_SOFT_OK;
}

constexpr int kPlanSlots = 4;
constexpr int kAuxStreams = 3;  // side streams for the launches of a batch that mixes window classes (see psk_soft_process_device)
constexpr int kStageSlots = 3;  // chunks of the host-buffer path in flight (< kPlanSlots)
constexpr int kQualitySlots = 4;  // calls whose quality pass (PSK_SOFT_OPT_QUALITY) may be in flight: descriptors and partials of each
constexpr int kAcquireSlots = 4;  // psk_soft_acquire_device calls that may be in flight: descriptors and partials of each
constexpr int kCvtScratch = 4;  // conversion scratch buffers of CS16 / CS8 / CF16 packets, one per stream that uses them (see StreamScratch)
constexpr int kGatherScratch = 4;  // gather scratch buffers of strided packets, one per stream that uses them (see StreamScratch)
constexpr int kGatherDescSlots = 4;  // strided calls whose gather descriptors may be in flight
// bytes of a packet's element
inline size_t elem_bytes(const psk_soft_packet_t &k)
{
    const psk::PktFormat *const f = psk::pkt_format(k.format);
    return f ? f->elem_bytes : sizeof(float);
}
// bytes of the upload slot of a call of n channels: header, plans, compact lists, CS16 / CS8 / CF16 conversion descriptors (psk_plan.h)
inline size_t slot_cvt_offset(size_t n)
{
    return (psk::kPlanHeaderBytes + (sizeof(psk::ChanPlan) + sizeof(uint32_t)) * n + 15u) & ~(size_t)15u;
}
// ... then one more channel list for the reference-order kernel when a call has CS16 / CS8 / CF16 channels on the in-place kernels:
// the channels of the float build, of the CS16 build, of the CS8 build, of the CF16 build (and of the wide-symbol build)
inline size_t slot_seq_offset(size_t n) { return slot_cvt_offset(n) + sizeof(psk::CvtDesc) * n; }
inline size_t slot_bytes(size_t n) { return slot_seq_offset(n) + sizeof(uint32_t) * n; }

// Minimal fork-join pool for the host-buffer path: packing packets into pinned memory and
// unpacking results are plain memcpy work that one thread cannot do at PCIe rate.
class CopyPool {
public:
    explicit CopyPool(int n_threads)
    {
        for (int t = 0; t < n_threads; t++) workers_.emplace_back([this] { loop(); });
    }
    ~CopyPool()
    {
        {
            std::lock_guard<std::mutex> g(m_);
            stop_ = true;
        }
        cv_.notify_all();
        for (auto &w : workers_) w.join();
    }
    // fn(i) for i in [0, n); the caller takes part; returns when all are done
    void run(uint32_t n, const std::function<void(uint32_t)> &fn)
    {
        if (!n)
            return;
        if (workers_.empty() || n == 1) {
            for (uint32_t i = 0; i < n; i++) fn(i);
            return;
        }
        {
            std::lock_guard<std::mutex> g(m_);
            fn_ = &fn;
            n_ = n;
            next_.store(0);
            busy_ = (int)workers_.size();
            gen_++;
        }
        cv_.notify_all();
        work();
        std::unique_lock<std::mutex> g(m_);
        done_.wait(g, [this] { return busy_ == 0; });
        fn_ = nullptr;
    }

private:
    void work()
    {
        for (;;) {
            uint32_t i = next_.fetch_add(1);
            if (i >= n_)
                break;
            (*fn_)(i);
        }
    }
    void loop()
    {
        uint64_t seen = 0;
        for (;;) {
            {
                std::unique_lock<std::mutex> g(m_);
                cv_.wait(g, [&] { return stop_ || gen_ != seen; });
                if (stop_)
                    return;
                seen = gen_;
            }
            work();
            {
                std::lock_guard<std::mutex> g(m_);
                if (--busy_ == 0)
                    done_.notify_all();
            }
        }
    }
    std::vector<std::thread> workers_;
    std::mutex m_;
    std::condition_variable cv_, done_;
    const std::function<void(uint32_t)> *fn_ = nullptr;
    uint32_t n_ = 0;
    std::atomic<uint32_t> next_{0};
    int busy_ = 0;
    uint64_t gen_ = 0;
    bool stop_ = false;
};

// One launch set of a call: the channels that go through the same launches, listed together in the compact lists behind the plans;
// first what the plan pass counts (account), then where and how the set runs (fill_lists, place_tiles).  Plain data, zeroed with the
// PlanSummary that holds it.
struct LaunchSet {
    uint64_t blocks;           // 128-symbol blocks of its calls, in all
    uint32_t cnt, max_blocks;  // channels; blocks of its longest call
    // LDS rings of a launch are sized for the largest phaseAvg / numAvg among its channels: a ring of
    // y_len unwrapped phases (a power of two >= phaseAvg + 128) and, for numAvg <= 128, an energy
    // ring of r_len positions (even, >= numAvg + 128)
    uint32_t max_n, max_A;
    uint32_t off;                    // where its list starts in the compact lists
    uint32_t tiles_max, pipe_tiles;  // time-tiled: tiles of its longest call; pipelined: tiles of a range
    uint16_t max_S;                  // largest samplesPerBaud (the sets without an instantiation)
    uint8_t K;                       // time-tiled: blocks to a tile
    bool tiled : 1, piped : 1;       // goes through the time-tiled kernels first; ... in ranges of tiles on three streams
};
static_assert(sizeof(LaunchSet) == 40, "PlanSummary is zeroed per call: no larger than the tables it replaced");

// What the control-plane pass over a batch found out: the first refusal, if any, and which kernels
// the accepted plans need.
struct PlanSummary {
    psk_soft_status st = PSK_SOFT_OK;
    uint32_t bad = 0;  // first refused channel (index into the batch)
    int why = 0;       // 0: status of plan_call, 2: alignment, 3: packet format
    bool any_plan = false, any_emit = false, any_seq = false;
    bool long_call = false;  // some channel's call is planned for the reference-order kernel only because of its length
    // The launch sets, in the order of their lists: the calls that emit nothing (max_n: of those whose window needs room in the launch's
    // LDS ring); the window classes without an instantiation (PLAN_ANYFRONT), one set for all of them; of them, the wide symbols
    // (samplesPerBaud > kSeqMaxS, psk_wide.hip); of both, the channels of the far fit (PLAN_FARFIT, phaseAvg > kFastFitMax), so that the
    // LDS rings of the two stay sized for their own channels; the far fit's calls that emit nothing while the window holds values
    // (psk_far_quiet_kernel); then the window classes of the wave-scan kernels, [samplesPerBaud][class, see kClassH]
    LaunchSet quiet{}, any{}, wide{}, anyf{}, widef{}, quietf{};
    LaunchSet cls[33][17]{};
};

// One chunk of channels of the host-buffer path in flight: pinned and device buffers for the packed
// packets and the packed four output streams, its own stream (so that the upload of one chunk, the
// kernels of another and the download of a third overlap), and an event for "outputs are in host
// memory".
struct StageSlot {
    Stream stream;
    Event done;
    PinnedBuf<uint8_t> h_buf;  // [in | soft | phase | bits | sidx]
    DeviceBuf<uint8_t> d_buf;
    size_t in_cap = 0;         // bytes of the input region; the others follow as IN, IN/2, IN, IN/4
    bool busy = false;
    // what the chunk in flight needs for unpacking
    uint32_t ch0 = 0, nch = 0;
    std::vector<size_t> off_soft, off_phase, off_bits, off_sidx;
    size_t soft_bytes = 0, phase_bytes = 0, bits_bytes = 0, sidx_bytes = 0;
};
inline size_t region_soft(size_t in_cap) { return in_cap; }
inline size_t region_phase(size_t in_cap) { return in_cap + in_cap; }
inline size_t region_bits(size_t in_cap) { return in_cap + in_cap + in_cap / 2; }
inline size_t region_sidx(size_t in_cap) { return in_cap + in_cap + in_cap / 2 + in_cap; }
inline size_t region_total(size_t in_cap) { return in_cap + in_cap + in_cap / 2 + in_cap + in_cap / 4; }
inline size_t align_up(size_t v, size_t a) { return (v + a - 1) / a * a; }
// Where the CS16 / CS8 / CF16 packets of a call are converted to (psk_pkt.hip: float2 rows) and where its strided packets are gathered to
// (psk_soft_process_device_strided, psk_gather.hip: rows in the packet's own element type): rows on 128-byte boundaries of a buffer
// grown on demand.  One buffer per stream that calls with such packets -- the chunks of psk_soft_process_host run on streams of their
// own and would otherwise wait for each other --; a buffer taken over from another stream is used behind the event that ends its last call.
struct StreamScratch {
    hipStream_t stream = nullptr;
    DeviceBuf<char> buf;
    size_t cap = 0;  // bytes
    Event ev;
    uint64_t last_use = 0;
};
// ... and the descriptors of one strided call (psk_gather.h): written into page-locked memory, uploaded on the caller's stream in
// front of the gather, reused behind the event that ends the call
struct GatherDescSlot {
    PinnedBuf<char> h_buf;
    DeviceBuf<char> d_buf;
    size_t cap = 0;  // bytes
    Event ev;
    // the slot for a call with `bytes` of descriptors: behind the event of its last call, grown on demand
    psk_soft_status claim(size_t bytes)
    {
        PSK_HIP(ev.ensure());
        PSK_HIP(ev.sync());
        ev.clear();
        if (bytes <= cap)
            return PSK_SOFT_OK;
        h_buf.release(), d_buf.release();
        cap = 0;
        const size_t grown = align_up(bytes + bytes / 4, 4096);
        PSK_HIP(h_buf.alloc(grown));
        PSK_HIP(d_buf.alloc(grown));
        cap = grown;
        return PSK_SOFT_OK;
    }
};
// The history of every channel in front of a pre-pass that needs one (the resampler's, the filter's): two slots a channel in
// device memory, allocated (zeros) when the first packet of the kind comes.  A launch reads the channel's current slot and
// writes the other; the call flips the two once ALL of it has succeeded, so a failed call leaves the history as it was.  The
// event is behind the last launch that read or wrote a slot.
struct HistoryBank {
    const char *name;                                  // in messages
    uint32_t slot_floats, chan_floats, live_floats;    // a slot, a channel's two slots with their padding, what of a slot is history
    DeviceBuf<float> d;
    std::vector<uint8_t> cur;  // the current slot of each channel
    Event ev;

    psk_soft_status ensure(uint32_t nch)
    {
        if (d)
            return PSK_SOFT_OK;
        PSK_TRY(alloc_zeroed(d, (size_t)chan_floats * nch, name));
        cur.assign(nch, 0);
        return PSK_SOFT_OK;
    }
    float *slot(uint32_t ch, uint32_t which) const { return d + (size_t)chan_floats * ch + slot_floats * which; }
    const float *in(uint32_t ch) const { return slot(ch, cur[ch]); }
    float *out(uint32_t ch) const { return slot(ch, cur[ch] ^ 1u); }
    void flip(uint32_t ch) { cur[ch] ^= 1u; }
    psk_soft_status record(hipStream_t stream)
    {
        PSK_HIP(ev.record(stream));
        return PSK_SOFT_OK;
    }
    // no launch is still reading or writing a slot
    psk_soft_status wait()
    {
        PSK_HIP(ev.sync());
        return PSK_SOFT_OK;
    }
    // the current slot of a channel, live_floats floats: zeros while nothing is allocated
    psk_soft_status get(uint32_t ch, float *to)
    {
        std::memset(to, 0, sizeof(float) * live_floats);
        if (!d)
            return PSK_SOFT_OK;
        if (const psk_soft_status st = wait())
            return st;
        PSK_HIP(hipMemcpy(to, in(ch), sizeof(float) * live_floats, hipMemcpyDeviceToHost));
        return PSK_SOFT_OK;
    }
    psk_soft_status set(uint32_t nch, uint32_t ch, const float *from)
    {
        if (const psk_soft_status st = ensure(nch))
            return st;
        if (const psk_soft_status st = wait())
            return st;
        PSK_HIP(hipMemcpy(slot(ch, cur[ch]), from, sizeof(float) * live_floats, hipMemcpyHostToDevice));
        return PSK_SOFT_OK;
    }
};

// ---- the reduction-pass layer: what the fold + join passes behind a call share ----
// A pass is a fold over pieces and a join per record on the caller's stream: PSK_SOFT_OPT_QUALITY's behind a process call
// (psk_quality.hip), the two looks (psk_acquire.hip, psk_symrate.hip), the word search (psk_sync.hip), the demapper (psk_demap.hip).
// An entry of the kind has a PassRing and a Records in the handle and goes through them in this order: next + claim a slot of the
// ring; fill the slot's pinned descriptors, one per record of the call, giving each its partials with a PieceCount (which holds the
// 2^31 limit; the message is the entry's); then run(): room for the partials, the descriptors up behind the passes of other streams
// that write the same records, the entry's own launches (its trace lines, its fold, its join, whatever else it puts on the stream),
// and the slot's event behind them however they ended.  Its psk_soft_get_* is its own argument check and records_read.  A pass
// over the handle's channels asks claim for the handle's channel count, so that its descriptors are allocated once, and covers
// the channels of its call; a pass over something else (the demapper's segments) asks for what the call needs and covers
// kAllRecords.  The chunks of psk_soft_process_host run on streams of their own and overlap, hence a ring of N slots.

// the records a pass writes: [first, first + n) of the entry's
struct PassCover {
    uint32_t first, n;
};
constexpr PassCover kAllRecords = {0u, UINT32_MAX};

// The partials of a pass, handed out as its descriptors are filled: where a record's start and how many it has; the pass's total
// and the most any record has.
struct PieceCount {
    uint64_t total = 0;
    uint32_t max_piece = 0;
    // a record of `pieces` pieces; false, and nothing counted: the pass would have 2^31 partials or more
    bool add(uint64_t pieces, uint32_t *part0, uint32_t *n_piece)
    {
        if (pieces > 0x7fffffffull || total + pieces > 0x7fffffffull)
            return false;
        *part0 = (uint32_t)total;
        *n_piece = (uint32_t)pieces;
        total += pieces;
        max_piece = *n_piece > max_piece ? *n_piece : max_piece;
        return true;
    }
};

// What a pass owns until its event: the descriptors (pinned, and their copy in device memory) and the partials of the fold, both
// grown on demand.  A pass goes through the members in the order they stand in.
template <class Desc, class Partial, int N>
struct PassRing {
    struct Slot {
        PinnedBuf<Desc> h_desc;
        DeviceBuf<Desc> d_desc;
        size_t desc_cap = 0;  // descriptors
        DeviceBuf<Partial> d_part;
        size_t part_cap = 0;  // partials
        Event ev;  // behind the slot's last pass
        hipStream_t stream = nullptr;
        PassCover cover = {0, 0};
    } slot[N];
    int turn = 0;

    // the slot of the next pass ...
    Slot &next()
    {
        Slot &q = slot[turn];
        turn = (turn + 1) % N;
        return q;
    }
    // ... once its last pass has ended, with room for n_desc descriptors: a slot that has less gets n_desc + headroom.  The event is
    // created on first use.
    static psk_soft_status claim(Slot &q, size_t n_desc, size_t headroom = 0)
    {
        PSK_HIP(q.ev.sync());
        q.ev.clear();  // (the event has completed: nothing waits for it again until finish records it for the next pass)
        PSK_HIP(q.ev.ensure());
        if (n_desc <= q.desc_cap)
            return PSK_SOFT_OK;
        q.h_desc.release(), q.d_desc.release();
        q.desc_cap = 0;
        PSK_HIP(q.h_desc.alloc(n_desc + headroom));
        PSK_HIP(q.d_desc.alloc(n_desc + headroom));
        q.desc_cap = n_desc + headroom;
        return PSK_SOFT_OK;
    }
    // room for n partials
    static psk_soft_status grow(Slot &q, uint64_t n)
    {
        if (n <= q.part_cap)
            return PSK_SOFT_OK;
        q.part_cap = 0;
        const size_t cap = with_headroom((size_t)n);
        PSK_HIP(q.d_part.alloc(cap));
        q.part_cap = cap;
        return PSK_SOFT_OK;
    }
    // A record is written by one pass at a time: `stream` waits for the passes of other streams over records of `cover`; then the
    // n_desc descriptors go up and the slot is the pass's.
    psk_soft_status upload(Slot &q, uint32_t n_desc, PassCover cover, hipStream_t stream)
    {
        for (const Slot &k : slot)
            if (&k != &q && k.stream != stream && k.cover.first < cover.first + cover.n && cover.first < k.cover.first + k.cover.n)
                PSK_HIP(k.ev.wait(stream));  // (a slot whose pass has been waited for, or that never had one: nothing)
        PSK_HIP(hipMemcpyAsync(q.d_desc, q.h_desc, sizeof(Desc) * (size_t)n_desc, hipMemcpyHostToDevice, stream));
        q.stream = stream, q.cover = cover;
        return PSK_SOFT_OK;
    }
    // The slot is free again behind whatever the pass has put on the stream.  Returns `st`, the pass's status so far (its error text
    // kept), or the failure to record.
    static psk_soft_status finish(Slot &q, hipStream_t stream, psk_soft_status st)
    {
        const std::string keep = g_last_error;
        if (const hipError_t e = q.ev.record(stream)) {  // (the slot stays as claim left it: nothing waits for its event)
            (void)hipStreamSynchronize(stream);
            if (st == PSK_SOFT_OK)
                return fail(PSK_SOFT_ERR_HIP, std::string("hipEventRecord: ") + hipGetErrorString(e));
        }
        g_last_error = keep;
        return st;
    }
    // The pass from its filled descriptors on: room for n_part partials, the descriptors up, then enqueue() -- the entry's launches,
    // a psk_soft_status -- and, on every path behind a successful upload, the slot's event.
    template <class Enqueue>
    psk_soft_status run(Slot &q, uint32_t n_desc, PassCover cover, uint64_t n_part, hipStream_t stream, Enqueue enqueue)
    {
        PSK_TRY(grow(q, n_part));
        PSK_TRY(upload(q, n_desc, cover, stream));
        return finish(q, stream, enqueue());
    }
    // every pass enqueued so far has ended
    psk_soft_status wait()
    {
        for (Slot &q : slot) PSK_HIP(q.ev.sync());
        return PSK_SOFT_OK;
    }
};

// The records of an entry, one per channel of the handle or per segment of the last call: an array in device memory, written by
// the joins; a control-plane-only handle keeps them on the host.
template <class Rec>
struct Records {
    DeviceBuf<Rec> d;
    size_t cap = 0;  // records of d
    std::vector<Rec> dry;

    bool exist() const { return d || !dry.empty(); }
    // n records of zeros, unless they exist (`what`: in the message of a failure)
    psk_soft_status ensure_zeroed(bool on_host, size_t n, const char *what)
    {
        if (on_host && dry.empty())
            dry.assign(n, Rec{});
        if (on_host || d)
            return PSK_SOFT_OK;
        PSK_TRY(alloc_zeroed(d, n, what));
        cap = n;
        return PSK_SOFT_OK;
    }
    // room for n records in device memory behind every pass of `ring`; what the records held is not kept
    template <class Ring>
    psk_soft_status grow(Ring &ring, size_t n)
    {
        if (n <= cap)
            return PSK_SOFT_OK;
        PSK_TRY(ring.wait());
        cap = 0;
        PSK_HIP(d.alloc(with_headroom(n)));
        cap = with_headroom(n);
        return PSK_SOFT_OK;
    }
};

// Largest phaseAvg of the wave-scan kernels: their LDS ring of unwrapped phases holds phaseAvg + 128 values in a power
// of two; 32768 floats (128 KiB) leave room for the energy ring next to it.  Channels with phaseAvg > kDeepFit are
// launched apart from the others of their window class ("deep" classes, index H + 8): a ring that size allows one wave
// per CU, and sized for the whole launch it would take the residency of thousands of ordinary channels with it.
constexpr uint32_t kFastFitMax = 32768 - 128;
constexpr uint32_t kDeepFit = 2048 - 128;
// second index of the per-class tables: history blocks (+ 8: deep fit window); 3: one block, CS16 packets read in place; 5: one
// block, CS8 packets read in place; 6: one block, CF16 packets read in place (psk_ctl.h: PktFormat::cls)
const int kClassH[] = {1, 3, 5, 6, 2, 4, 8, 9, 10, 12, 16};
// the format whose packets class Hi reads in place; nullptr: a class of the float kernels
inline const psk::PktFormat *class_pkt(int Hi)
{
    for (const psk::PktFormat &f : psk::kPktFormats)
        if (f.cls == Hi)
            return &f;
    return nullptr;
}
inline int class_H(int Hi) { return class_pkt(Hi) ? 1 : Hi > 8 ? Hi - 8 : Hi; }
constexpr uint32_t in_place_flags()
{
    uint32_t m = 0;
    for (const psk::PktFormat &f : psk::kPktFormats) m |= f.in_place;
    return m;
}
constexpr uint32_t kInPlaceFlags = in_place_flags();
constexpr int kNumClassH = (int)(sizeof(kClassH) / sizeof(kClassH[0]));
// time-tiled kernels, automatic choice (measured, tools/tiled_sweep2.sh: QPSK, samplesPerBaud 8): a class of at most 64
// channels whose longest call has at least 16 blocks of 128 symbols, or of at most 512 channels and 192 blocks (at 128
// blocks the two paths are level there; above 512 channels the wave-scan kernels fill the machine by themselves);
// tiles of 2 .. 16 blocks, as many as make kTiledTargetTiles tiles
constexpr uint32_t kTiledFewChannels = 64, kTiledMinBlocksFew = 16, kTiledMaxChannels = 512, kTiledMinBlocks = 192;
constexpr uint64_t kTiledTargetTiles = 4096;
// the pipelined mode of the time-tiled path (front / fit / back of consecutive ranges of tiles on three streams, psk_tile.hip:
// psk_tile_fit_range_kernel): window classes of a few hundred to a few thousand channels with long calls
constexpr uint32_t kPipeMinChannels = 288, kPipeMaxChannels = 1408, kPipeMinBlocks = 256, kPipeMaxRanges = 32, kPipeMaxYLen = 1024;
constexpr size_t kPipeMaxSymbols = (size_t)1 << 29;  // (16 bytes of scratch a symbol: 8 GiB)
constexpr int kPipeEvents = 2 * (int)kPipeMaxRanges + 2;
// a batch of several window classes whose calls are at least this long is cut in time (psk_soft_process_device)
constexpr uint32_t kSplitMinBlocks = 128;
constexpr uint32_t kSeqMaxS = 1024;    // symbolEnergy[] of the reference-order kernel lives in LDS; wider symbols: psk_wide.hip and
                                       // the PSK_SEQ_WIDE build of that kernel
const int kFastS[] = {2,  3,  4,  5,  6,  7,  8,  9,  10, 11, 12, 13, 14, 15, 16, 17,
                      18, 19, 20, 21, 22, 23, 24, 25, 26, 27, 28, 29, 30, 31, 32};

}  // namespace

struct psk_soft_handle {
    int device = PSK_SOFT_DEVICE_NONE;
    bool dry = true;
    uint32_t nch = 0;
    psk::Limits lim{};
    psk_soft_limits_t user{};
    std::vector<psk::ChanCtl> ctl;
    std::vector<psk::ChanCtl> ctl_next;     // scratch of one call: planned on copies, committed on success
    std::vector<psk::ChanPlan> plans_dry;   // plans of a control-plane-only handle (no pinned slots)
    std::vector<uint32_t> last_mode;  // PlanMode of the last call, per channel (statistics)
    // Uniform run of the control plane (the stamped path of process_round): the channels [uni_lo, uni_hi) are known to hold
    // IDENTICAL control state.  While `lazy` is set that state lives in the run's ctl / mode alone and ctl[] / last_mode[] of
    // the range are stale: every reader goes through ctl_sync() first, every writer through ctl_touch().
    // A few such runs are kept side by side (disjoint): a caller that feeds a handle in two or four slices on as many streams --
    // so that the tail of one slice's launch overlaps the body of the next's -- keeps all of them stamped.
    struct UniRun {
        uint32_t lo = 0, hi = 0;
        bool lazy = false;
        psk::ChanCtl ctl;
        uint32_t mode = psk::PLAN_SKIP;
    };
    static constexpr int kUniRuns = 8;
    UniRun uni[kUniRuns];
    uint32_t mixed_lo = 0, mixed_hi = 0;  // a range that was compared and found mixed ...
    int mixed_ttl = 0;                    // ... is not compared again for this many calls (or until something is configured)
    int opt_stamp = 1;                    // PSK_SOFT_STAMP=0 (environment): every channel planned on its own (A/B runs, tests)
    // Every resource below is an owning member (DeviceBuf, PinnedBuf, Event, Stream: see "ownership" above) and goes with the handle.
    // psk_soft_destroy waits for every stream the handle owns before it deletes the handle, so nothing is in flight when the first
    // member goes and the order in which the members are destroyed does not matter.
    // device memory
    DeviceBuf<psk::ChanState> d_state;
    DeviceBuf<float2> d_ring;
    DeviceBuf<float> d_yv;
    // the plan slots: a pinned block and its copy in device memory; the plans lie kPlanHeaderBytes into each (psk_plan.h)
    PinnedBuf<char> h_plan_blk[kPlanSlots];
    DeviceBuf<char> d_plan_blk[kPlanSlots];
    psk::ChanPlan *h_plans[kPlanSlots] = {};
    psk::ChanPlan *d_plans[kPlanSlots] = {};
    Event ev[kPlanSlots];
    // the plans of a call are uploaded on a stream of their own, so that the copy runs under the kernels of the call before
    // instead of behind them (20 us of a 4096-channel call); the caller's stream waits for ev_up of the slot
    Stream up_stream;
    Event ev_up[kPlanSlots];
    int opt_up_stream = 1;  // PSK_SOFT_PLAN_STREAM=0 (environment): upload on the caller's stream (A/B runs)
    int slot = 0;
    bool opt_qpsk_sign_map = false;  // PSK_SOFT_OPT_QPSK_SIGN_BITMAP
    Stream stream;
    Stream aux[kAuxStreams];     // created on first use
    Event aux_fork, aux_join[kAuxStreams];
    int opt_fork = 1;                       // PSK_SOFT_OPT_CONCURRENT_CLASSES
    // PSK_SOFT_OPT_DEFERRED_JOIN: the side streams of a batch that mixes window classes are NOT joined into the caller's stream at
    // the end of the call -- every class ends its calls on its own stream (exact tier and reference-order hand-over included) and
    // the next call's launches of the class queue behind them there, so that a short class runs ahead into the next calls while a
    // long one is still busy.  The caller's stream sees the results after psk_soft_join() / psk_soft_synchronize().  Safe as long
    // as every channel keeps going to the same stream: the channel -> stream assignment of a call is hashed (deferred_sig), and
    // a call whose assignment differs from the pending one joins everything first.
    int opt_deferred = 0;
    bool deferred_pending = false;
    uint64_t deferred_sig = 0;
    uint32_t deferred_ch0 = 0, deferred_nch = 0;
    hipStream_t deferred_stream = nullptr;
    Event slot_aux_ev[kPlanSlots][kAuxStreams];  // end of a deferred call on each side stream (a plan slot is reused after them too)
    // what the call that last used each plan slot worked on, and on which stream (its end is the slot's event)
    hipStream_t slot_stream[kPlanSlots] = {};
    uint32_t slot_ch0[kPlanSlots] = {}, slot_nch[kPlanSlots] = {};
    // time-tiled kernels (psk_tile_kernel.h): scratch of one call -- per-tile reports, and per symbol the raw phase, the
    // picked sample and the phase estimate -- grown on demand; calls that use it on different streams are ordered by tile_ev
    int opt_tiled = 1;  // PSK_SOFT_OPT_TIME_TILED
    DeviceBuf<psk::TileInfo> d_tiles;
    DeviceBuf<float> d_traw, d_test;
    DeviceBuf<float2> d_ts;
    size_t tile_cap = 0, tile_sym_cap = 0;
    size_t pf_cap = 0, pf_sym_cap = 0;  // ... of the parallel fit's arrays (the classes that use it come first in the scratch)
    psk::PfScratch pf{};   // ... and of the parallel fit (psk_pfit.h), same capacities; PfChan: one per channel of the handle
    struct PfMem {         // what pf points at: the owner of its arrays and of its pinned note; scratch_tiles takes pf from view()
        DeviceBuf<int> k;
        DeviceBuf<float> y, tt;
        DeviceBuf<double> S, c, xs;
        DeviceBuf<psk::PfTile> tile;
        DeviceBuf<psk::PfBlock> blk;
        DeviceBuf<psk::PfWalk> walk;
        DeviceBuf<psk::PfChan> chan;
        PinnedBuf<uint32_t> hint;
        psk::PfScratch view() const { return psk::PfScratch{k, y, S, c, tt, xs, tile, blk, walk, chan, hint}; }
    } pf_mem;
    int opt_pfit = 1;      // PSK_SOFT_PARALLEL_FIT (environment): 0 = time-tiled calls keep the block-by-block fit (A/B runs),
                           // 2 = the second round of the parallel fit is always enqueued (tests), 1 = for a while after
                           // a call reported a first guess that failed (pf.hint, a word the kernels write into page-locked memory)
    int pf_second_ttl = 0;  // tiled calls left with the second round enqueued
    int opt_ties_in_place = 1;              // PSK_SOFT_TIES_IN_PLACE=0 (environment): PLAN_TIES_HANDOVER in every plan (tests, A/B runs)
    int opt_trace = 0;                      // PSK_SOFT_TRACE_LAUNCHES=1 (environment, debugging): see trace_launch
    int opt_validate = 0;                   // PSK_SOFT_VALIDATE=1 (environment, tests): see `validate` in process_round
    int opt_split = 2;                      // PSK_SOFT_SPLIT_CLASSES=n (environment): pieces a mixed batch's calls are cut into (0 / 1: never)
    int opt_pipe = 1;                       // PSK_SOFT_PIPELINED=0 (environment): never the pipelined mode (A/B runs)
    Stream pipe_st[2];                      // its fit and back streams (the front stage stays on the class's stream)
    Event pipe_ev[kPipeEvents];
    DeviceBuf<char> d_pipe_carry;           // per channel of a pipelined launch: the fit state between two ranges (PipeCarry)
    DeviceBuf<float> d_pipe_y;              // ... and its ring of unwrapped phases
    size_t pipe_cap = 0;
    // wide symbols (samplesPerBaud > kSeqMaxS): the chunk records of the front stage (psk_wide.hip) and the rows of symbolEnergy[] of the
    // reference-order kernel's wide build, grown on demand like the scratch above and ordered by the same event
    DeviceBuf<char> d_wide_rec, d_wide_stat;
    size_t wide_rec_cap = 0, wide_stat_cap = 0;  // bytes
    DeviceBuf<double> d_wide_symE;
    size_t wide_symE_cap = 0;  // doubles
    Event tile_ev;
    hipStream_t tile_stream = nullptr;  // stream of the last call that used the scratch
    // PSK_SOFT_OPT_FAR_FIT: phaseAvg above kFastFitMax on the fast path (psk_farfit.hip).  The rings of that fit stage are rows of
    // d_far_y, one per channel that has ever emitted as a far channel (far_row[channel] = row + 1, 0: none yet) -- by channel, not by
    // position in the call: calls on disjoint channel ranges run side by side on different streams.  Grown on demand, never shrunk;
    // a row holds nothing between calls (the prologue of every call copies the carried values in).
    int opt_far_fit = 0;
    DeviceBuf<float> d_far_y;
    uint32_t far_rows_cap = 0, far_rows_used = 0;
    std::vector<uint32_t> far_row;
    bool poisoned = false;  // a HIP call failed after kernels of a call were enqueued: host mirror and device state may disagree
    // CS16 / CS8 / CF16 packets: conversion scratch (StreamScratch)
    StreamScratch cvt[kCvtScratch];
    uint64_t cvt_calls = 0;
    // strided packets: gather scratch and descriptor slots (StreamScratch, GatherDescSlot)
    StreamScratch gat[kGatherScratch];
    GatherDescSlot gdesc[kGatherDescSlots];
    uint64_t gat_calls = 0;
    int gdesc_turn = 0;
    DeviceBuf<float> d_tune_tab;  // tuned packets: the two phasor tables (psk_tune.h), uploaded when the first tuned packet comes
    // resampled packets: the history of every channel, two slots of three float2 in 64 bytes
    HistoryBank rs_hist{"resample history", psk::kResampleHistSlotFloats, psk::kResampleHistFloats, psk::kResampleHistSlotFloats};
    // filtered packets: the taps of every slot (kFirSlots x kFirMaxTaps floats, allocated at the first psk_soft_fir_define) and
    // their counts (0: never defined); the history of every channel, two slots of 127 float2 in 1 KiB each
    DeviceBuf<float> d_fir_taps;
    uint32_t fir_ntaps[psk::kFirSlots] = {};
    HistoryBank fir_hist{"filter history", psk::kFirHistSlotFloats, 2u * psk::kFirHistSlotFloats, 2u * psk::kFirHist};
    int opt_diag_gather_only = 0;  // PSK_SOFT_DIAG_GATHER_ONLY=1 (environment, timing experiments only -- tools/strided_rates.py): a
                                   // strided call gathers and returns; the ordinary call behind it is left out, outs[] untouched
    // PSK_SOFT_OPT_QUALITY: one record per channel, written by the pass behind every call (psk_quality.hip); a control-plane-only
    // handle keeps them on the host
    int opt_quality = 0;
    Records<psk_soft_quality_t> quality;
    PassRing<psk::QualityDesc, psk::QualityPartial, kQualitySlots> qpass;
    struct QualitySnap {
        uint16_t M, S;
        uint8_t diff;
    };
    std::vector<QualitySnap> q_snap;  // scratch of one call: the properties it ran with
    // psk_soft_acquire_device: one record per channel, written by the join of the last call that covered it (psk_acquire.hip); a
    // control-plane-only handle keeps them on the host
    Records<psk_soft_acquire_t> acquire;
    PassRing<psk::AcquireDesc, psk::AcquirePartial, kAcquireSlots> apass;
    // psk_soft_symrate_device: the same for the symbol-rate look (psk_symrate.hip)
    Records<psk_soft_symrate_t> symrate;
    PassRing<psk::SymrateDesc, psk::SymratePartial, kAcquireSlots> spass;
    // psk_soft_sync_device: the words of every slot (kSyncSlots x kSyncMaxWord float2, allocated at the first psk_soft_sync_define),
    // their lengths (0: never defined) and energies Ew; one record per channel, allocated (zeros) at the first call -- a
    // control-plane-only handle keeps them on the host --; the history of every channel, two slots of 127 float2 in 1 KiB each
    DeviceBuf<float> d_sync_words;
    uint32_t sync_len[psk::kSyncSlots] = {};
    float sync_ew[psk::kSyncSlots] = {};
    Records<psk_soft_sync_t> sync;
    PassRing<psk::SyncDesc, psk::SyncPartial, kAcquireSlots> ypass;
    HistoryBank sync_hist{"sync history", psk::kSyncHistSlotFloats, 2u * psk::kSyncHistSlotFloats, 2u * psk::kSyncHist};
    // ... and what PSK_SOFT_DEMAP_FRONT asks of a channel: how the last sync call that covered it left it (empty: no call yet)
    enum : uint8_t { kSyncNotSearched = 0, kSyncSearched = 1, kSyncSearchedRestart = 2 };
    std::vector<uint8_t> sync_last;
    // psk_soft_demap_device: the maps of every slot (kDemapSlots DemapMap, allocated at the first psk_soft_demap_define; M 0: never
    // defined); one record per segment of the last call, grown on demand -- a control-plane-only handle keeps them on the host --;
    // the passes' descriptors grow on demand too, and every pass covers all the records (kAllRecords)
    DeviceBuf<psk::DemapMap> d_demap_maps;
    uint32_t demap_M[psk::kDemapSlots] = {};
    Records<psk_soft_demap_t> demap;
    bool demap_called = false;
    uint32_t demap_nseg = 0;    // of the last call
    PassRing<psk::DemapDesc, psk::DemapPartial, 2> dpass;
    // psk_soft_viterbi_device: the codes of every slot (kViterbiSlots ViterbiCode, allocated at the first psk_soft_viterbi_define;
    // K 0: never defined) and their copy on the host; one record per frame of the last call, grown on demand -- a
    // control-plane-only handle keeps them on the host --; the "partials" of its pass are the decision words of the frames in
    // flight (psk_viterbi.hip), at most kViterbiScratchWords a call
    DeviceBuf<psk::ViterbiCode> d_viterbi_codes;
    psk::ViterbiCode viterbi_code[psk::kViterbiSlots] = {};
    Records<psk_soft_viterbi_t> viterbi;
    bool viterbi_called = false;
    uint32_t viterbi_nframe = 0;  // of the last call
    PassRing<psk::ViterbiDesc, uint64_t, 2> vpass;
    // psk_soft_rs_device: the codes of every slot (kRsSlots RsCode, allocated at the first psk_soft_rs_define; gfpoly 0: never
    // defined), their masks (kRsMaskStride bytes a slot) and the codes' copy on the host; one record per frame of the last call,
    // grown on demand -- a control-plane-only handle keeps them on the host --; its pass has no partials
    DeviceBuf<psk::RsCode> d_rs_codes;
    DeviceBuf<uint8_t> d_rs_masks;
    psk::RsCode rs_code[psk::kRsSlots] = {};
    Records<psk_soft_rs_t> rs;
    bool rs_called = false;
    uint32_t rs_nframe = 0;  // of the last call
    PassRing<psk::RsDesc, uint32_t, 2> rpass;
    // psk_soft_frame_search_device: the words of every slot (on the host: a stream's descriptor carries its word; length 0: never
    // defined); one record per stream of the last call; a ring of two passes with the fold's partials.
    psk::FrameWord frame_word[psk::kFrameSlots] = {};
    Records<psk_soft_frame_search_t> fsearch;
    bool fsearch_called = false;
    uint32_t fsearch_n = 0;  // streams of the last call
    PassRing<psk::FrameSearchDesc, psk::FrameSearchPartial, 2> fpass;
    // psk_soft_frame_cut_device: the formats of every slot (branches 0: never defined), their tables (256 bytes a slot, allocated
    // with the first table; a control-plane-only handle keeps none); one record per frame of the last call; a ring of its own
    // without partials.
    psk::FrameFormat frame_format[psk::kFrameSlots] = {};
    DeviceBuf<uint8_t> d_frame_tables;
    Records<psk_soft_frame_cut_t> fcut;
    bool fcut_called = false;
    uint32_t fcut_n = 0;  // frames of the last call
    PassRing<psk::FrameCutDesc, uint32_t, 2> cpass;
    // ingest pipeline of the host-buffer entry point (psk_soft_process_host)
    StageSlot stage[kStageSlots];
    std::unique_ptr<CopyPool> pool;
    size_t stage_bytes = 32u << 20;  // input bytes per chunk (PSK_SOFT_STAGE_MB)
};

namespace {
// the per-channel mirror of one run brought up to date (see psk_soft_handle::UniRun)
void run_sync(psk_soft_handle *h, psk_soft_handle::UniRun &r)
{
    if (!r.lazy)
        return;
    for (uint32_t i = r.lo; i < r.hi; i++) {
        h->ctl[i] = r.ctl;
        h->last_mode[i] = r.mode;
    }
    r.lazy = false;
}
// ... of the whole handle
void ctl_sync(const psk_soft_handle *hc)
{
    psk_soft_handle *h = const_cast<psk_soft_handle *>(hc);
    for (auto &r : h->uni) run_sync(h, r);
}
// ... and about to be changed channel by channel: nothing is known to be uniform any more
void ctl_touch(psk_soft_handle *h)
{
    for (auto &r : h->uni) {
        run_sync(h, r);
        r.lo = r.hi = 0;
    }
    h->mixed_lo = h->mixed_hi = 0;
    h->mixed_ttl = 0;
}
// ... of the channels [lo, hi), which are about to be planned one by one: the runs that overlap them end
void ctl_touch_range(psk_soft_handle *h, uint32_t lo, uint32_t hi)
{
    for (auto &r : h->uni)
        if (r.hi > r.lo && r.lo < hi && lo < r.hi) {
            run_sync(h, r);
            r.lo = r.hi = 0;
        }
}
// the run that is exactly [lo, hi), or none
psk_soft_handle::UniRun *run_find(psk_soft_handle *h, uint32_t lo, uint32_t hi)
{
    for (auto &r : h->uni)
        if (r.hi > r.lo && r.lo == lo && r.hi == hi)
            return &r;
    return nullptr;
}
// PSK_SOFT_OPT_DEFERRED_JOIN: `stream` waits for everything the side streams still carry
hipError_t deferred_join(psk_soft_handle *h, hipStream_t stream)
{
    if (!h->deferred_pending)
        return hipSuccess;
    for (int a = 0; a < kAuxStreams; a++) {
        if (!h->aux[a])
            continue;
        if (const hipError_t e = h->aux_join[a].record(h->aux[a]))
            return e;
        if (const hipError_t e = h->aux_join[a].wait(stream))
            return e;
    }
    h->deferred_pending = false;
    return hipSuccess;
}
// the control state of one channel, wherever it lives at the moment (nothing is brought up to date)
const psk::ChanCtl &ctl_of(const psk_soft_handle *h, uint32_t c)
{
    for (const auto &r : h->uni)
        if (r.lazy && r.lo <= c && c < r.hi)
            return r.ctl;
    return h->ctl[c];
}
bool ctl_equal(const psk::ChanCtl &a, const psk::ChanCtl &b)
{
    return a.props.samplesPerBaud == b.props.samplesPerBaud && a.props.constelationSize == b.props.constelationSize &&
           a.props.numAvg == b.props.numAvg && a.props.phaseAvg == b.props.phaseAvg &&
           a.props.differentialDecoding == b.props.differentialDecoding && a.props.resetState == b.props.resetState &&
           a.resetSamplesPerBaud == b.resetSamplesPerBaud && a.resetNumSymbols == b.resetNumSymbols && a.resetPhaseAvg == b.resetPhaseAvg &&
           a.ring_len == b.ring_len && a.symEnergySize == b.symEnergySize && a.index == b.index && a.count == b.count &&
           std::memcmp(&a.sampleRate, &b.sampleRate, sizeof(float)) == 0 && a.lf_n == b.lf_n &&
           std::memcmp(&a.lf_xdelta, &b.lf_xdelta, sizeof(float)) == 0 && a.lf_len == b.lf_len && a.lf_count == b.lf_count &&
           a.lf_head == b.lf_head && a.ring_src == b.ring_src && a.lf_recompute_pending == b.lf_recompute_pending;
}

// ---- one pass of the control plane over a batch and the launches it asks for: process_round and its phases ----

struct Cls { int S, H; };  // a window class of the call
// What a round works on: what it was called with, where its plans and lists live, what the plan pass found out (res), and what each
// phase leaves for the ones behind it.
struct Round {
    psk_soft_handle *h;
    uint32_t ch0, nch;
    const psk_soft_packet_t *pkts;
    psk_soft_output_t *outs;
    const uint8_t *cont;  // pieces of a call the library has cut, see process_round
    bool of_split;        // ... of a mixed batch cut in time: the side streams are not joined between its rounds
    hipStream_t stream;
    int slot;
    bool dry;
    uint32_t extra_flags;
    psk::Limits lim;
    psk::ChanPlan *plans = nullptr;
    uint32_t *handed_over = nullptr;  // (psk_plan.h)
    bool stamped = false;             // the stamped path: one plan and one copy of the control state stand for the range
    psk::ChanCtl stamp_ctl;
    psk_soft_handle::UniRun *run = nullptr;
    PlanSummary res;
    uint32_t *h_list = nullptr;  // compact lists, one per launch set, behind the plans
    const uint32_t *d_list = nullptr;
    const psk::ChanPlan *d_plans = nullptr;  // (the plans and lists as the kernels see them)
    uint32_t far_rows = 0;  // channels of anyf, widef and quietf: the three lists follow one another
    // the scratch of the time-tiled kernels: symbols and tiles placed, of them the parallel fit's, what the wide symbols and the pipeline need
    size_t tile_syms = 0, tile_count = 0, pf_syms = 0, pf_count = 0, wide_rec_need = 0, wide_stat_need = 0, pipe_need = 0;
    uint32_t wide_z = 0, n_wide_seq = 0, wide_seq_S = 0;  // (n_wide_seq: channels of the reference-order kernel's wide build)
    bool pf_second = false;
    // conversion pre-pass: descriptors in all and per format, the longest packet of each, the scratch they convert into
    uint32_t n_cvt = 0, n_cvt_f[psk::kNumPktFormats] = {};
    uint64_t cvt_max_n[psk::kNumPktFormats] = {};
    StreamScratch *cv = nullptr;
    uint32_t n_in_place = 0, n_in_place_f[psk::kNumPktFormats] = {}, n_seq_narrow = 0;  // the reference-order kernel's lists
    Cls cls[33 * kNumClassH];  // the schedule
    int n_cls = 0;
    bool fork = false, deferred = false;
    uint64_t sig = 0;
};
// (a phase that fails ends the round with its status: PSK_TRY)

// CS16, CS8 and CF16 channels of the window classes with in-place instantiations (psk_fast_inst.hip, PSK_INST_PKT): a class of
// their own per format, no conversion.  (What would go through the time-tiled kernels is moved back: move_in_place_back.)
bool in_place(const psk::ChanPlan &p, const psk::PktFormat &f)
{
    return (p.lf_flags & f.flag) && p.mode == psk::PLAN_FAST && p.n_out && !(p.lf_flags & psk::PLAN_ANYFRONT) && p.A <= 128u &&
           p.lf_n <= kDeepFit && psk::fast_pkt_has((int)f.id, (int)p.S);
}
// the class of a planned channel that emits on the wave-scan kernels
int class_of(const psk::ChanPlan &p)
{
    for (const psk::PktFormat &f : psk::kPktFormats)
        if (p.lf_flags & f.in_place)
            return f.cls;
    return psk::fast_hist_blocks(p.A) + (p.lf_n > kDeepFit ? 8 : 0);
}
// The launch set a planned channel belongs to; nullptr: the reference-order kernel.  The one place that decides it: the plan pass
// counts with it (account), the compact lists are filled with it (fill_lists).
LaunchSet *set_of(const psk::ChanPlan &p, const psk::Limits &lim, PlanSummary &r)
{
    if (p.mode != psk::PLAN_FAST)
        return nullptr;
    if (p.n_out && (p.lf_flags & psk::PLAN_FARFIT))
        return p.S > kSeqMaxS ? &r.widef : &r.anyf;
    if (p.n_out && (p.lf_flags & psk::PLAN_ANYFRONT))
        return p.S > kSeqMaxS ? &r.wide : &r.any;
    if (p.n_out)
        return &r.cls[p.S][class_of(p)];
    if (lim.far_fit && p.lf_n > lim.fast_fit_max && p.lf_len0)
        return &r.quietf;  // (nothing emitted, but prologue and epilogue go through the window: no LDS holds it)
    return &r.quiet;
}
// f(set) for every launch set in the order of the lists: quiet, any, wide, anyf, widef, quietf, then the classes
template <class F>
void each_set(PlanSummary &r, F f)
{
    for (LaunchSet *s : {&r.quiet, &r.any, &r.wide, &r.anyf, &r.widef, &r.quietf}) f(*s);
    for (int S : kFastS)
        for (int H : kClassH) f(r.cls[S][H]);
}
// what a planned channel asks of the launches (`mult` channels with this very plan)
void account(psk::ChanPlan &p, const psk::Limits &lim, PlanSummary &r, uint32_t mult)
{
    r.any_plan = true;
    for (const psk::PktFormat &f : psk::kPktFormats)  // (read in place: the channel joins the class of its format)
        if (in_place(p, f))
            p.lf_flags |= f.in_place;
    LaunchSet *const s = set_of(p, lim, r);
    if (!s) {
        r.any_seq = true;
        if (!lim.force_seq && p.lf_n <= (lim.far_fit ? 65535u : lim.fast_fit_max) &&
            (p.n_out > psk::kResyncCount || (uint64_t)p.lf_count0 + p.n_out > psk::kResyncCount))
            r.long_call = true;
        return;
    }
    s->cnt += mult;
    if (!p.n_out) {
        // (an empty far window needs no room in the launch's LDS ring: nothing is copied in or out)
        if (s == &r.quiet && p.lf_n > s->max_n && (p.lf_len0 || p.lf_n <= lim.fast_fit_max)) s->max_n = p.lf_n;
        return;
    }
    r.any_emit = true;
    const uint32_t nb = (uint32_t)((p.n_out + 127u) / 128u);
    s->blocks += (uint64_t)nb * mult;
    if (nb > s->max_blocks) s->max_blocks = nb;
    if (p.lf_n > s->max_n) s->max_n = p.lf_n;
    if (p.A > s->max_A) s->max_A = p.A;
    if (p.S > s->max_S) s->max_S = (uint16_t)p.S;
}
// (packet data: 8-byte aligned float pairs, 4-byte aligned int16 and binary16 pairs, 2-byte aligned int8 pairs)
bool misaligned(const Round &r, const psk::ChanPlan &p)
{
    uintptr_t in_mask = 7u;
    for (const psk::PktFormat &f : psk::kPktFormats)
        if (p.lf_flags & f.flag)
            in_mask = f.align_mask;
    return !r.dry && ((p.n_in && !p.in) || ((uintptr_t)p.in & in_mask) || ((uintptr_t)p.soft & 7u) || ((uintptr_t)p.bits & 3u) ||
                      ((uintptr_t)p.phase & 3u) || ((uintptr_t)p.sidx & 3u));
}
// The plans are written straight into the pinned upload slot of this call: wait until the launch
// that last used the slot has consumed it.  (A refused call does not advance the slot.)
psk_soft_status take_slot(Round &r)
{
    psk_soft_handle *const h = r.h;
    if (h->dry) {
        if (h->plans_dry.size() < r.nch)
            h->plans_dry.resize(r.nch);
        r.plans = h->plans_dry.data();
        return PSK_SOFT_OK;
    }
    PSK_HIP(hipSetDevice(h->device));
    PSK_HIP(h->ev[r.slot].sync());
    for (Event &e : h->slot_aux_ev[r.slot]) {  // (a deferred call's classes end on the side streams)
        PSK_HIP(e.sync());
        e.clear();
    }
    r.plans = h->h_plans[r.slot];
    r.handed_over = psk::plan_header(h->d_plans[r.slot]);
    return PSK_SOFT_OK;
}
// ---- the stamped path ----
// Channels configured alike and fed packets of the same length ever since hold IDENTICAL control state, and a batch of equal packets
// gets the same plan in every channel but for its five pointers: planned ONCE, stamped into the other slots, the new control state
// kept in ONE copy that stands for the range until somebody looks at a single channel (ctl_sync).  Per channel: ~3 ns against ~14 ns.
// Anything unusual -- a refused call, a packet that differs, a buffer too small or misaligned -- leaves for the ordinary path.
//
// the run that stands for [ch0, ch0 + nch), found or newly made; nullptr: the channels are not known to be alike
psk_soft_handle::UniRun *uniform_run(psk_soft_handle *h, uint32_t ch0, uint32_t nch)
{
    if (psk_soft_handle::UniRun *const run = run_find(h, ch0, ch0 + nch))
        return run;
    ctl_touch_range(h, ch0, ch0 + nch);  // (runs that overlap the range without being it)
    if (h->mixed_ttl > 0 && h->mixed_lo == ch0 && h->mixed_hi == ch0 + nch) {  // (known to be mixed)
        h->mixed_ttl--;
        return nullptr;
    }
    const psk::ChanCtl &c0 = h->ctl[ch0];
    for (uint32_t i = 1; i < nch; i++)
        if (!ctl_equal(c0, h->ctl[ch0 + i])) {
            h->mixed_lo = ch0, h->mixed_hi = ch0 + nch, h->mixed_ttl = 256;
            return nullptr;
        }
    psk_soft_handle::UniRun *run = nullptr;
    for (int k = psk_soft_handle::kUniRuns - 1; k >= 0; k--)  // (the first free slot)
        run = h->uni[k].hi == h->uni[k].lo ? &h->uni[k] : run;
    if (!run) {  // (every slot taken: the first one makes room)
        run = &h->uni[0];
        run_sync(h, *run);
    }
    run->lo = ch0, run->hi = ch0 + nch, run->lazy = false;
    return run;
}
// plans the batch the stamped way if it can (r.stamped); if it cannot, nothing of the attempt is left in r.res
void plan_stamped(Round &r)
{
    psk_soft_handle *const h = r.h;
    if (!h->opt_stamp || r.cont || r.nch < 16u || !(r.run = uniform_run(h, r.ch0, r.nch)))
        return;
    r.stamp_ctl = r.run->lazy ? r.run->ctl : h->ctl[r.ch0];
    psk::ChanPlan &p0 = r.plans[0];
    const psk_soft_packet_t &k0 = r.pkts[0];
    if (psk::plan_call(r.stamp_ctl, r.lim, k0, r.outs[0], p0, false) != PSK_SOFT_OK || p0.mode == psk::PLAN_SKIP || misaligned(r, p0))
        return;
    p0.lf_flags |= r.extra_flags;
    p0.handed_over = r.handed_over;
    account(p0, r.lim, r.res, r.nch);
    const psk_soft_output_t o0 = r.outs[0];
    uint32_t i = 1;
    for (const uint32_t n = r.res.long_call ? 0u : r.nch; i < n; i++) {
        const psk_soft_packet_t &k = r.pkts[i];
        psk_soft_output_t &o = r.outs[i];
        if (k.n_floats != k0.n_floats || k.format != k0.format || k.present != k0.present || k.sri_mode != k0.sri_mode || k.sriChanged != k0.sriChanged ||
            k.inputQueueFlushed != k0.inputQueueFlushed || std::memcmp(&k.sri_xdelta, &k0.sri_xdelta, sizeof(double)) != 0)
            break;
        if (p0.n_out > o.cap_symbols && (o.soft || o.bits || o.phase || o.sampleIndex))  // (plan_call's rule)
            break;
        psk::ChanPlan &p = r.plans[i];
        p = p0;
        p.in = k.data, p.soft = o.soft, p.bits = o.bits, p.phase = o.phase, p.sidx = o.sampleIndex;
        if (misaligned(r, p))
            break;
        o.ret = o0.ret, o.n_symbols = o0.n_symbols, o.n_bits = o0.n_bits, o.n_sampleIndex = o0.n_sampleIndex;
        o.sri_pushed = o0.sri_pushed, o.sri_soft_xdelta = o0.sri_soft_xdelta, o.sri_bits_xdelta = o0.sri_bits_xdelta;
        o.n_warn = o0.n_warn;
    }
    r.stamped = i == r.nch;
    if (!r.stamped)
        r.res = PlanSummary();
}
// The ordinary path: every channel planned on its own, on copies (ctl_next); committed only if every channel of the batch is accepted.
// One thread: ~15 ns per channel; a thread pool was measured and dropped (waking the workers costs more than the whole pass).
void plan_each(Round &r)
{
    psk::ChanCtl *const next = r.h->ctl_next.data() + r.ch0;
    const psk::ChanCtl *const cur = r.h->ctl.data() + r.ch0;
    PlanSummary &res = r.res;
    for (uint32_t i = 0; i < r.nch; i++) {
        next[i] = cur[i];
        psk::ChanPlan &p = r.plans[i];
        psk_soft_status st = psk::plan_call(next[i], r.lim, r.pkts[i], r.outs[i], p, r.cont && (r.cont[i] & 1u));
        if (st != PSK_SOFT_OK) {
            res.st = st, res.bad = i, res.why = st == PSK_SOFT_ERR_INVALID_ARG ? 3 : 0;
            return;
        }
        if (p.mode == psk::PLAN_SKIP)
            continue;
        if (misaligned(r, p)) {
            res.st = PSK_SOFT_ERR_INVALID_ARG, res.bad = i, res.why = 2;
            return;
        }
        p.lf_flags |= r.extra_flags;
        p.handed_over = r.handed_over;
        if (r.cont && (r.cont[i] & 2u))
            p.lf_flags |= psk::PLAN_NO_WRAP;  // (more pieces of this call follow)
        if (r.cont && (r.cont[i] & 4u))
            p.lf_flags |= psk::PLAN_CARRY_DRIFT;  // (a piece cut where the reference does not rebuild its sums)
        account(p, r.lim, res, 1u);
    }
}
// the refusal the plan pass found, as the caller gets it
psk_soft_status refusal(const Round &r)
{
    const PlanSummary &res = r.res;
    if (res.why == 2)
        return fail(PSK_SOFT_ERR_INVALID_ARG,
                    "psk_soft_process: packet data must be 8-byte aligned (CS16: 4) (CS8: 2) (CF16: 4), soft 8, bits 4, phase 4, sampleIndex 4");
    char buf[160];
    if (res.why == 3) {
        std::snprintf(buf, sizeof buf, "psk_soft_process: channel %u: unknown packet format %u (PSK_SOFT_FORMAT_CF32 = 0, CS16 = 1, CS8 = 3, CF16 = 4)",
                      r.ch0 + res.bad, (unsigned)r.pkts[res.bad].format);
        return fail(PSK_SOFT_ERR_INVALID_ARG, buf);
    }
    std::snprintf(buf, sizeof buf, "psk_soft_process: channel %u refused (status %d)", r.ch0 + res.bad, (int)res.st);
    return fail(res.st, buf);
}
// The host mirror (ctl) is committed only once everything the call needs has been enqueued: a HIP error before the first kernel launch
// leaves the channels untouched; one after it poisons the handle (device state half advanced, nothing to roll it back with).
void commit(Round &r)
{
    psk_soft_handle *const h = r.h;
    if (r.stamped) {  // (one copy stands for the range: see ctl_sync)
        r.run->ctl = r.stamp_ctl;
        r.run->mode = r.plans[0].mode;
        r.run->lazy = true;
        return;
    }
    if (r.ch0 == 0 && r.nch == h->nch)
        h->ctl.swap(h->ctl_next);
    else
        std::memcpy(static_cast<void *>(h->ctl.data() + r.ch0), h->ctl_next.data() + r.ch0, sizeof(psk::ChanCtl) * r.nch);
    for (uint32_t i = 0; i < r.nch; i++) h->last_mode[r.ch0 + i] = r.plans[i].mode;
}
// Calls that touch the same channels must run in order: a call waits for the earlier calls on OTHER streams whose channel range overlaps
// its own (same stream: the stream orders them; older calls than the plan slots remember have completed -- a slot is only reused after its event).
psk_soft_status wait_for_overlapping_calls(Round &r)
{
    psk_soft_handle *const h = r.h;
    for (int k = 0; k < kPlanSlots; k++)
        if (k != r.slot && h->ev[k].recorded() && h->slot_stream[k] != r.stream && h->slot_ch0[k] < r.ch0 + r.nch &&
            r.ch0 < h->slot_ch0[k] + h->slot_nch[k]) {
            PSK_HIP(h->ev[k].wait(r.stream));
            for (const Event &e : h->slot_aux_ev[k]) PSK_HIP(e.wait(r.stream));
        }
    return PSK_SOFT_OK;
}
// CS16, CS8 and CF16 channels read in place have classes of their own (PktFormat::cls), which have no
// time-tiled kernels: where the float class would go through those (the same choice as in place_all, on the four classes together),
// their channels go back to the float class and to the conversion pre-pass
void move_in_place_back(Round &r)
{
    const psk_soft_handle *const h = r.h;
    if (r.stamped && !(r.plans[0].lf_flags & kInPlaceFlags))
        return;
    for (int S = 2; S <= 16; S++) {
        LaunchSet &fl = r.res.cls[S][1];
        uint32_t cnt = fl.cnt, mb = fl.max_blocks, mn = fl.max_n;
        for (const psk::PktFormat &f : psk::kPktFormats) {
            const LaunchSet &c = r.res.cls[S][f.cls];
            cnt += c.cnt;
            mb = c.max_blocks > mb ? c.max_blocks : mb;
            mn = c.max_n > mn ? c.max_n : mn;
        }
        if (cnt == fl.cnt || !h->opt_tiled || !psk::tile_front_has(S, 1))  // (no channel read in place, or no time-tiled kernels)
            continue;
        const bool pipe = h->opt_pipe == 2 ? mb >= 4u
                                           : h->opt_pipe && h->opt_tiled == 1 && cnt >= kPipeMinChannels && cnt <= kPipeMaxChannels &&
                                                 mb >= kPipeMinBlocks && !r.cont && mn + 128u <= kPipeMaxYLen;
        const bool tiled = h->opt_tiled == 2 || pipe || (cnt <= kTiledFewChannels && mb >= kTiledMinBlocksFew) ||
                           (cnt <= kTiledMaxChannels && mb >= kTiledMinBlocks);
        if (!tiled)
            continue;
        fl.cnt = cnt, fl.max_blocks = mb, fl.max_n = mn;
        for (const psk::PktFormat &f : psk::kPktFormats) {
            LaunchSet &c = r.res.cls[S][f.cls];
            fl.max_A = fl.max_A > c.max_A ? fl.max_A : c.max_A;
            fl.blocks += c.blocks;
            c = LaunchSet{};
        }
        for (uint32_t i = 0; i < r.nch; i++)
            if (r.plans[i].S == (uint32_t)S)
                r.plans[i].lf_flags &= ~kInPlaceFlags;
    }
}
// compact lists, one per launch set, behind the plans: first the channels that emit nothing, then the sets without an
// instantiation, then every (S, H) class
void fill_lists(Round &r)
{
    r.h_list = reinterpret_cast<uint32_t *>(r.h->h_plans[r.slot] + r.nch);
    r.d_plans = r.h->d_plans[r.slot];
    r.d_list = reinterpret_cast<const uint32_t *>(r.d_plans + r.nch);
    uint32_t run = 0;
    each_set(r.res, [&](LaunchSet &s) {
        s.off = run;
        run += s.cnt;
    });
    r.far_rows = r.res.anyf.cnt + r.res.widef.cnt + r.res.quietf.cnt;
    // (stamped: one set holds every channel, in order; the offsets of the others are equal to its end -- unless the stamped class was
    // just moved back to the float class: its offsets are that class's then, the lists the same)
    if (r.stamped) {
        for (uint32_t i = 0; i < r.nch; i++) r.h_list[i] = i;
        return;
    }
    for (uint32_t i = 0; i < r.nch; i++)  // (`off` runs along as the set's list fills ...)
        if (LaunchSet *const s = set_of(r.plans[i], r.lim, r.res))
            r.h_list[s->off++] = i;
    each_set(r.res, [](LaunchSet &s) { s.off -= s.cnt; });  // (... and goes back to its start)
}
struct TileRule {  // how a launch set is cut into tiles: the four things in which the sets differ
    uint64_t k_min;  // the least blocks to a tile: 1 for the wide symbols (few symbols a call fill the machine only on short tiles), else 2
    uint32_t z;      // tiles are counted in waves: a wave per chunk of 1024 timing phases for the wide symbols (wide_z), else 1
    bool lengthen;   // towards the longest window, which the front stage rebuilds in front of a tile; the window classes keep short tiles
    bool pfit;       // full fit windows take the parallel fit (never the far fit, whose window is in device memory; never a pipelined class)
};
// The set goes through the time-tiled kernels (psk_tile_kernel.h): its channels get a place in the scratch of the call -- symbols
// padded to whole blocks, K blocks to a tile, K chosen so that the set makes a few thousand tiles.
void place_tiles(Round &r, LaunchSet &s, const TileRule &rule)
{
    const uint64_t blocks_z = s.blocks * rule.z;
    uint64_t K = blocks_z / kTiledTargetTiles;
    K = K < rule.k_min ? rule.k_min : K > 16 ? 16 : K;
    // (a tile rebuilds the window in front of it: tiles at least as long as the longest window keep that a fraction of the
    // work -- where there are tiles enough to fill the machine anyway; a few channels finish sooner on many short tiles)
    const uint64_t k_win = (s.max_A + 127u) / 128u;
    if (rule.lengthen && K < k_win) {
        const uint64_t k_fill = blocks_z / (kTiledTargetTiles / 2);
        const uint64_t k_long = k_win > 64 ? 64 : k_win;
        K = k_fill > k_long ? k_long : k_fill > K ? k_fill : K;
    }
    s.tiled = true;
    s.K = (uint8_t)K;
    s.tiles_max = (uint32_t)((s.max_blocks + K - 1) / K);
    for (uint32_t i = 0; i < s.cnt; i++) {
        psk::ChanPlan &p = r.plans[r.h_list[s.off + i]];
        const uint64_t nb = (p.n_out + 127u) / 128u;
        p.lf_flags |= psk::PLAN_TILED;
        if (rule.pfit && r.h->opt_pfit && p.lf_len0 == p.lf_n && p.lf_n >= 2)
            p.lf_flags |= psk::PLAN_PFIT;
        p.tile_blocks = (uint32_t)K;
        p.tile_base = (uint32_t)r.tile_count;
        p.tile_off = r.tile_syms;
        r.tile_count += (size_t)((nb + K - 1) / K);
        r.tile_syms += (size_t)nb * 128u;
    }
}
// a pipelined class that has its tiles: the tiles of a range
void place_ranges(Round &r, LaunchSet &s)
{
    s.piped = true;
    const uint32_t T = s.tiles_max;
    uint32_t tr = (uint32_t)(kTiledTargetTiles / s.cnt);  // (a range = about one machine-load of tiles)
    tr = tr < 1u ? 1u : tr;
    if (r.h->opt_pipe == 2 && tr > 3u)
        tr = 3u;
    if (const char *e = std::getenv("PSK_SOFT_PIPE_RANGE_TILES"))  // (A/B runs)
        tr = std::atoi(e) > 0 ? (uint32_t)std::atoi(e) : tr;
    if ((T + tr - 1) / tr > kPipeMaxRanges)
        tr = (T + kPipeMaxRanges - 1) / kPipeMaxRanges;
    s.pipe_tiles = tr;
    if (s.off + s.cnt > r.pipe_need)
        r.pipe_need = s.off + s.cnt;
}
// Every set that goes through the time-tiled kernels gets its place in the scratch.  The order matters: the wide symbols first -- their
// places index the chunk records of psk_wide.hip too, which need not cover the others --, then the other sets without an instantiation, then
// the window classes of few channels and long calls; the pipelined ones last -- the parallel fit's scratch need not cover them.
void place_all(Round &r)
{
    const psk_soft_handle *const h = r.h;
    PlanSummary &res = r.res;
    r.wide_z = (res.wide.cnt || res.widef.cnt) ? psk::wide_chunks(res.wide.max_S > res.widef.max_S ? res.wide.max_S : res.widef.max_S) : 0u;
    // (the sets without an instantiation: always tiled, whatever the option says -- the alternative is the reference-order kernel)
    if (res.wide.cnt)
        place_tiles(r, res.wide, TileRule{1, r.wide_z, true, true});
    if (res.widef.cnt)
        place_tiles(r, res.widef, TileRule{1, r.wide_z, true, false});
    r.wide_rec_need = r.tile_syms * r.wide_z * psk::wide_rec_bytes(), r.wide_stat_need = r.tile_count * r.wide_z * psk::wide_stat_bytes();
    if (res.any.cnt)
        place_tiles(r, res.any, TileRule{2, 1, true, true});
    if (res.anyf.cnt)
        place_tiles(r, res.anyf, TileRule{2, 1, true, false});
    r.pf_syms = r.tile_syms, r.pf_count = r.tile_count;
    for (int pass = 0; pass < (h->opt_tiled ? 2 : 0); pass++) {
        for (int S : kFastS)
            for (int H : kClassH) {
                LaunchSet &s = res.cls[S][H];
                if (!s.cnt || class_pkt(H) || !psk::tile_front_has(S, class_H(H)))
                    continue;
                // pipelined: the serial fit of a range under the front stage of the next (see kPipeMinChannels)
                // (PSK_SOFT_PIPELINED=2, tests: wherever the kernels allow it, a few blocks to a range)
                const bool pipe = (h->opt_pipe == 2 ? s.max_blocks >= 4u
                                                    : h->opt_pipe && h->opt_tiled == 1 && s.cnt >= kPipeMinChannels && s.cnt <= kPipeMaxChannels &&
                                                          s.max_blocks >= kPipeMinBlocks) &&
                                  !r.cont && s.max_n + 128u <= kPipeMaxYLen && (size_t)s.blocks * 128u <= kPipeMaxSymbols;
                if (pipe != (pass == 1))
                    continue;
                if (!pipe && h->opt_tiled == 1 &&
                    !((s.cnt <= kTiledFewChannels && s.max_blocks >= kTiledMinBlocksFew) || (s.cnt <= kTiledMaxChannels && s.max_blocks >= kTiledMinBlocks)))
                    continue;
                place_tiles(r, s, TileRule{2, 1, false, !pipe});
                if (pipe)
                    place_ranges(r, s);
            }
        if (pass == 0)
            r.pf_syms = r.tile_syms, r.pf_count = r.tile_count;
    }
}

struct ScratchBuf {  // one buffer of a scratch that grows on demand, and the bytes it is to have
    OwnedBytes<DeviceMem> *buf;
    size_t bytes;
};
template <class T>
inline ScratchBuf scratch_buf(DeviceBuf<T> &b, size_t n) { return ScratchBuf{&b, sizeof(T) * n}; }
inline size_t plus_quarter(size_t need) { return need + need / 4; }  // (a scratch grows to the largest call seen, plus a quarter)
// A scratch is too small for the call (rare): the device is waited for -- no call is in flight on a buffer that moves --, the buffers
// are freed and allocated anew.  *got = false: out of device memory, none of them is held; what the call does then is the caller's business.
hipError_t grow_scratch(std::initializer_list<ScratchBuf> bufs, bool *got)
{
    if (const hipError_t e = hipDeviceSynchronize())
        return e;
    for (const ScratchBuf &b : bufs) b.buf->release();
    *got = true;
    for (const ScratchBuf &b : bufs) *got = *got && b.buf->alloc_bytes(b.bytes) == hipSuccess;
    if (!*got) {
        (void)hipGetLastError();
        for (const ScratchBuf &b : bufs) b.buf->release();
    }
    return hipSuccess;
}
// The scratch of `ring` for a call on `stream` that needs `need` bytes of it: the stream's own buffer, else the one used longest ago;
// `stream` waits for the event that ends the buffer's last call on another stream; a buffer too small grows to the need plus a quarter, in
// whole pages (rare: the one place that waits for the device).  Out of device memory: `oom`, or without one the plain HIP error.
template <int N>
psk_soft_status claim_scratch(StreamScratch (&ring)[N], uint64_t *calls, hipStream_t stream, size_t need, const char *oom, StreamScratch **out)
{
    StreamScratch *sc = &ring[0], *own = nullptr;
    for (StreamScratch &c : ring) {
        sc = c.last_use < sc->last_use ? &c : sc;
        own = !own && c.buf && c.stream == stream ? &c : own;
    }
    *out = sc = own ? own : sc;
    PSK_HIP(sc->ev.ensure());
    if (sc->stream != stream)
        PSK_HIP(sc->ev.wait(stream));
    if (need > sc->cap) {
        sc->cap = 0;
        const size_t cap = align_up(plus_quarter(need), 4096);
        if (oom) {
            bool got = false;
            PSK_HIP(grow_scratch({scratch_buf(sc->buf, cap)}, &got));
            if (!got)
                return fail(PSK_SOFT_ERR_HIP, oom);
        } else {
            PSK_HIP(hipDeviceSynchronize());
            PSK_HIP(sc->buf.alloc(cap));
        }
        sc->cap = cap;
    }
    sc->stream = stream, sc->last_use = ++*calls;
    return PSK_SOFT_OK;
}
// the channel's call goes to the reference-order kernel after all
void to_reference_order(psk::ChanPlan &p)
{
    p.mode = p.S == 1u ? psk::PLAN_SEQ_S1 : psk::PLAN_SEQ;
    p.lf_flags &= ~(uint32_t)(psk::PLAN_TILED | psk::PLAN_PFIT | psk::PLAN_ANYFRONT | psk::PLAN_FARFIT);
}
// the scratch of the time-tiled kernels and of the parallel fit
psk_soft_status scratch_tiles(Round &r)
{
    psk_soft_handle *const h = r.h;
    PlanSummary &res = r.res;
    if (!r.tile_syms || (r.tile_syms <= h->tile_sym_cap && r.tile_count <= h->tile_cap && r.pf_syms <= h->pf_sym_cap && r.pf_count <= h->pf_cap))
        return PSK_SOFT_OK;
    h->tile_cap = h->tile_sym_cap = h->pf_cap = h->pf_sym_cap = 0;
    const size_t syms = plus_quarter(r.tile_syms), cnt = plus_quarter(r.tile_count);
    const size_t psyms = plus_quarter(r.pf_syms) + 128u, pcnt = plus_quarter(r.pf_count) + 1u;
    psk_soft_handle::PfMem &pf = h->pf_mem;
    bool got = false;
    PSK_HIP(grow_scratch({scratch_buf(h->d_tiles, cnt), scratch_buf(h->d_traw, syms), scratch_buf(h->d_test, syms), scratch_buf(h->d_ts, syms),
                          scratch_buf(pf.k, psyms), scratch_buf(pf.y, psyms), scratch_buf(pf.S, psyms), scratch_buf(pf.c, psyms),
                          scratch_buf(pf.tt, psyms), scratch_buf(pf.xs, psyms), scratch_buf(pf.tile, pcnt),
                          scratch_buf(pf.blk, psyms / 128u + 1u), scratch_buf(pf.walk, psyms / 128u + 1u)},
                         &got));
    if (got && !pf.chan) {
        got = pf.chan.alloc(h->nch) == hipSuccess && hipMemset(pf.chan, 0, sizeof(psk::PfChan) * h->nch) == hipSuccess &&
              pf.hint.alloc(16) == hipSuccess;  // (64 bytes)
        if (got)
            *pf.hint = 0u;
    }
    h->pf = pf.view();  // (whatever moved or went: the kernels' struct follows its owner)
    if (got) {
        h->tile_cap = cnt, h->tile_sym_cap = syms, h->pf_cap = pcnt, h->pf_sym_cap = psyms;
        return PSK_SOFT_OK;
    }
    (void)hipGetLastError();
    // (out of device memory: the call does without -- the wave-scan kernels carry everything on their own)
    for (uint32_t i = 0; i < r.nch; i++) {
        psk::ChanPlan &p = r.plans[i];
        if (p.lf_flags & psk::PLAN_ANYFRONT) {  // (no kernel but the reference-order one is left for these)
            to_reference_order(p);
            res.any_seq = true;
        }
        p.lf_flags &= ~(uint32_t)(psk::PLAN_TILED | psk::PLAN_PFIT);
    }
    res.any.cnt = res.wide.cnt = res.anyf.cnt = res.widef.cnt = 0;
    for (int S : kFastS)
        for (int H : kClassH) res.cls[S][H].tiled = res.cls[S][H].piped = false;
    r.tile_syms = 0;
    return PSK_SOFT_OK;
}
// the chunk records of the wide front stage
psk_soft_status scratch_wide(Round &r)
{
    psk_soft_handle *const h = r.h;
    PlanSummary &res = r.res;
    if (!(res.wide.cnt || res.widef.cnt) || (r.wide_rec_need <= h->wide_rec_cap && r.wide_stat_need <= h->wide_stat_cap))
        return PSK_SOFT_OK;
    h->wide_rec_cap = h->wide_stat_cap = 0;
    const size_t rb = plus_quarter(r.wide_rec_need), sb = plus_quarter(r.wide_stat_need);
    bool got = false;
    PSK_HIP(grow_scratch({scratch_buf(h->d_wide_rec, rb), scratch_buf(h->d_wide_stat, sb)}, &got));
    if (got) {
        h->wide_rec_cap = rb, h->wide_stat_cap = sb;
        return PSK_SOFT_OK;
    }
    // (out of device memory: the reference-order kernel carries these calls)
    for (const LaunchSet *s : {&res.wide, &res.widef})
        for (uint32_t i = 0; i < s->cnt; i++) to_reference_order(r.plans[r.h_list[s->off + i]]);
    res.wide.cnt = res.widef.cnt = 0;
    res.any_seq = true;
    return PSK_SOFT_OK;
}
// the far fit's rings: a row of the scratch for every channel of its launch sets (kept from the channel's first such call on);
// anyf, widef and quietf are walked as one range of the lists
psk_soft_status scratch_far_rows(Round &r)
{
    psk_soft_handle *const h = r.h;
    PlanSummary &res = r.res;
    if (!r.far_rows)
        return PSK_SOFT_OK;
    const uint32_t *const list = r.h_list + res.anyf.off;
    if (h->far_row.empty())
        h->far_row.assign(h->nch, 0u);
    uint32_t used = h->far_rows_used;
    for (uint32_t i = 0; i < r.far_rows; i++)
        if (!h->far_row[r.ch0 + list[i]])
            used++;
    bool got = true;
    if (used > h->far_rows_cap) {
        // (the one place of this path that waits for the device: a row carries nothing from one call to the next)
        h->far_rows_cap = 0;
        const uint32_t cap = plus_quarter(used) < h->nch ? (uint32_t)plus_quarter(used) : h->nch;
        PSK_HIP(grow_scratch({ScratchBuf{&h->d_far_y, psk::far_ring_bytes() * cap}}, &got));
        if (got)
            h->far_rows_cap = cap;
    }
    for (uint32_t i = 0; i < r.far_rows; i++) {
        psk::ChanPlan &p = r.plans[list[i]];
        if (got) {
            uint32_t &row = h->far_row[r.ch0 + list[i]];
            if (!row)
                row = ++h->far_rows_used;
            p.far_row = row - 1u;
        } else if (p.n_out) {  // (out of device memory: the reference-order kernel carries these calls, as with the option off)
            to_reference_order(p);
        }
    }
    if (!got) {
        if (res.quietf.cnt)  // (... but a call that emits nothing has no other kernel to go to)
            return fail(PSK_SOFT_ERR_HIP, "psk_soft_process: out of device memory for the fit window of a far channel (PSK_SOFT_OPT_FAR_FIT)");
        res.anyf.cnt = res.widef.cnt = 0;
        res.any_seq = true;
    }
    return PSK_SOFT_OK;
}
// the reference-order kernel's wide build (samplesPerBaud > kSeqMaxS): a list of its own -- the other build's symbolEnergy[] is
// kSeqMaxS long -- and a row of symbolEnergy[] in device memory for each channel of it, as long as the widest
psk_soft_status scratch_wide_seq(Round &r)
{
    psk_soft_handle *const h = r.h;
    for (uint32_t i = 0; i < r.nch; i++)
        if (r.plans[i].mode != psk::PLAN_SKIP && r.plans[i].S > kSeqMaxS) {
            r.n_wide_seq++;
            r.wide_seq_S = r.plans[i].S > r.wide_seq_S ? r.plans[i].S : r.wide_seq_S;
        }
    const size_t need = (size_t)r.n_wide_seq * r.wide_seq_S;
    if (need <= h->wide_symE_cap)
        return PSK_SOFT_OK;
    h->wide_symE_cap = 0;
    bool got = false;
    PSK_HIP(grow_scratch({scratch_buf(h->d_wide_symE, plus_quarter(need))}, &got));
    if (!got)  // (nothing else carries a wide symbol)
        return fail(PSK_SOFT_ERR_HIP, "psk_soft_process: out of device memory for the symbolEnergy rows of wide symbols");
    h->wide_symE_cap = plus_quarter(need);
    return PSK_SOFT_OK;
}
// The scratch is one per handle: calls that use it on different streams are ordered by tile_ev (the rows of symbolEnergy[] are
// ordered like the scratch of the time-tiled kernels).  With it go the note of the parallel fit and the pipelined mode's own scratch.
psk_soft_status scratch_order(Round &r)
{
    psk_soft_handle *const h = r.h;
    if (!r.tile_syms && !r.n_wide_seq)
        return PSK_SOFT_OK;
    PSK_HIP(h->tile_ev.ensure());
    if (r.tile_syms) {
        // second round of the parallel fit: for the next 16 tiled calls after one whose first guess of the unwrap counts
        // failed somewhere (the kernels leave a note in page-locked memory; a late or lost note costs a call or two)
        if (h->pf.hint && *static_cast<volatile uint32_t *>(h->pf.hint)) {
            *static_cast<volatile uint32_t *>(h->pf.hint) = 0u;
            h->pf_second_ttl = 16;
        } else if (h->pf_second_ttl) {
            h->pf_second_ttl--;
        }
        r.pf_second = h->opt_pfit == 2 || h->pf_second_ttl > 0;
    }
    if (h->tile_stream != r.stream)
        PSK_HIP(h->tile_ev.wait(r.stream));
    if (!r.tile_syms || !r.pipe_need)
        return PSK_SOFT_OK;
    // the pipelined mode's own scratch (one PipeCarry and one ring of kPipeMaxYLen floats per channel of a launch) and its
    // two streams -- of another priority than the caller's, so that they get hardware queues of their own
    if (r.pipe_need > h->pipe_cap) {
        h->pipe_cap = 0;
        const size_t cap = plus_quarter(r.pipe_need);
        bool got = false;
        PSK_HIP(grow_scratch({scratch_buf(h->d_pipe_carry, psk::pipe_carry_bytes() * cap), scratch_buf(h->d_pipe_y, kPipeMaxYLen * cap)}, &got));
        if (got)
            h->pipe_cap = cap;
        else  // (out of device memory: the one-launch kernels do without)
            for (int S : kFastS)
                for (int H : kClassH) r.res.cls[S][H].piped = false;
    }
    if (!h->pipe_st[0]) {
        int prio_lo = 0, prio_hi = 0;
        PSK_HIP(hipDeviceGetStreamPriorityRange(&prio_lo, &prio_hi));
        // (CU-masked streams for the stages -- the serial ones on every n-th CU, the front stage on the others -- were measured:
        // no gain, 2.77 ... 2.84 against 2.75 ms at 512 channels)
        for (Stream &q : h->pipe_st) PSK_HIP(q.create(prio_hi));
        for (Event &e : h->pipe_ev) PSK_HIP(e.ensure());
    }
    return PSK_SOFT_OK;
}
// (the row in kPktFormats of a packet the pre-pass converts, else -1)
int cvt_format(const psk::ChanPlan &p)
{
    if (p.mode == psk::PLAN_SKIP || !p.n_in)
        return -1;
    for (int f = 0; f < psk::kNumPktFormats; f++)
        if ((p.lf_flags & psk::kPktFormats[f].flag) && !(p.lf_flags & psk::kPktFormats[f].in_place))
            return f;
    return -1;
}
// CS16, CS8 and CF16 packets (psk_pkt.hip): converted into float2 rows of the conversion scratch by one pre-pass per
// format in front of the call's first kernel; their plans point at the rows from here on.  The descriptors travel behind the
// plans, in the same upload: the CS16 packets' first, then the CS8 packets', then the CF16 packets' (the order of kPktFormats).
psk_soft_status conversion_descriptors(Round &r)
{
    psk_soft_handle *const h = r.h;
    size_t need = 0;
    for (uint32_t i = 0; i < r.nch; i++)
        if (const int f = cvt_format(r.plans[i]); f >= 0) {
            need += align_up(sizeof(float2) * r.plans[i].n_in, 128);
            r.n_cvt++, r.n_cvt_f[f]++;
        }
    if (!r.n_cvt)
        return PSK_SOFT_OK;
    // (without the scratch the call fails: nothing else reads these packets)
    PSK_TRY(claim_scratch(h->cvt, &h->cvt_calls, r.stream, need, "psk_soft_process: out of device memory for the conversion of CS16 / CS8 / CF16 packets",
                          &r.cv));
    const StreamScratch *const cv = r.cv;
    psk::CvtDesc *const desc =
        reinterpret_cast<psk::CvtDesc *>(reinterpret_cast<char *>(psk::plan_header(h->h_plans[r.slot])) + slot_cvt_offset(r.nch));
    size_t off = 0;
    uint32_t next[psk::kNumPktFormats] = {};  // (where each format's descriptors go on)
    for (int f = 1; f < psk::kNumPktFormats; f++) next[f] = next[f - 1] + r.n_cvt_f[f - 1];
    for (uint32_t i = 0; i < r.nch; i++) {
        psk::ChanPlan &p = r.plans[i];
        const int f = cvt_format(p);
        if (f < 0)
            continue;
        const uint32_t k = next[f]++;
        desc[k].src = reinterpret_cast<const uint32_t *>(p.in);
        desc[k].dst = reinterpret_cast<float *>(cv->buf + off);
        desc[k].n = p.n_in;
        p.in = desc[k].dst;
        off += align_up(sizeof(float2) * p.n_in, 128);
        r.cvt_max_n[f] = p.n_in > r.cvt_max_n[f] ? p.n_in : r.cvt_max_n[f];
    }
    return PSK_SOFT_OK;
}
// the reference-order kernel's lists when CS16 / CS8 / CF16 channels are read in place: float-build channels first, then the
// CS16 build's, then the CS8 build's, then the CF16 build's (and the wide symbols' last)
void reference_order_lists(Round &r)
{
    for (uint32_t i = 0; i < r.nch; i++)
        for (int f = 0; f < psk::kNumPktFormats; f++) r.n_in_place_f[f] += (r.plans[i].lf_flags & psk::kPktFormats[f].in_place) ? 1u : 0u;
    for (const uint32_t n : r.n_in_place_f) r.n_in_place += n;
    r.n_seq_narrow = r.nch - r.n_in_place - r.n_wide_seq;
    if (!r.n_in_place && !r.n_wide_seq)
        return;
    uint32_t *const seq = reinterpret_cast<uint32_t *>(reinterpret_cast<char *>(psk::plan_header(r.h->h_plans[r.slot])) + slot_seq_offset(r.nch));
    uint32_t a = 0, b[psk::kNumPktFormats] = {r.n_seq_narrow}, c = r.nch - r.n_wide_seq;
    for (int f = 1; f < psk::kNumPktFormats; f++) b[f] = b[f - 1] + r.n_in_place_f[f - 1];
    for (uint32_t i = 0; i < r.nch; i++) {
        uint32_t *at = &a;
        for (int f = 0; f < psk::kNumPktFormats; f++)
            if (r.plans[i].lf_flags & psk::kPktFormats[f].in_place)
                at = &b[f];
        if (r.plans[i].mode != psk::PLAN_SKIP && r.plans[i].S > kSeqMaxS)
            at = &c;
        seq[(*at)++] = i;
    }
}
// what PSK_SOFT_VALIDATE finds wrong with a plan, or nullptr
const char *invalid_plan(const Round &r, const psk::ChanPlan &p)
{
    const psk_soft_handle *const h = r.h;
    const uint64_t S = p.S ? p.S : 1u, have = (uint64_t)p.ring_len0 + p.n_in;
    const uint64_t nb = (p.n_out + 127u) / 128u;
    const bool emits = p.mode == psk::PLAN_FAST && p.n_out;
    const uint64_t tiles_end = p.tile_blocks ? (uint64_t)p.tile_base + (nb + p.tile_blocks - 1u) / p.tile_blocks : 0u;
    if (p.n_out && p.S > 1u && (p.n_out + p.A - 1u) * S > have)
        return "the call reads samples behind the packet's end";
    if (p.n_out && p.S <= 1u && p.mode != psk::PLAN_SEQ_S1 && p.n_out > p.n_in)
        return "more symbols than samples at one sample per symbol";
    if (p.ring_len0 > h->lim.ring_cap || p.ring_len1 > h->lim.ring_cap || p.ring_src > 1u)
        return "carried samples beyond the ring";
    if (p.ring_len1 > have)
        return "more samples carried out of the call than it holds";
    if (p.lf_n >= h->lim.fit_cap || p.lf_len0 > p.lf_n || p.lf_head >= h->lim.fit_cap)
        return "LinearFit window beyond its ring";
    if ((p.lf_flags & psk::PLAN_TILED) && emits && (!p.tile_blocks || p.tile_off + nb * 128u > h->tile_sym_cap || tiles_end > h->tile_cap))
        return "place in the time-tiled scratch outside it";
    if ((p.lf_flags & psk::PLAN_FARFIT) && emits &&
        (!h->d_far_y || p.far_row >= h->far_rows_cap || (p.lf_flags & psk::PLAN_PFIT) || p.lf_n < 128u))
        return "far fit without a row of its scratch";
    if ((p.lf_flags & psk::PLAN_PFIT) && emits && (p.tile_off + nb * 128u > h->pf_sym_cap || tiles_end > h->pf_cap))
        return "place in the parallel fit's scratch outside it";
    if (emits && !(p.lf_flags & psk::PLAN_ANYFRONT) && (p.S < 2u || p.S > 32u || p.A > 1024u || (p.S > 16u && p.A > 512u)))
        return "window class without a wave-scan instantiation planned for one";
    if (p.mode == psk::PLAN_FAST && p.n_out > psk::kResyncCount)
        return "a piece longer than 2^20 symbols on the wave-scan kernels";
    if ((p.lf_flags & psk::PLAN_TILED) && (p.lf_flags & psk::PLAN_ANYFRONT) && p.S > kSeqMaxS && emits &&
        (psk::wide_chunks(p.S) > r.wide_z || (p.tile_off + nb * 128u) * r.wide_z * psk::wide_rec_bytes() > h->wide_rec_cap ||
         tiles_end * r.wide_z * psk::wide_stat_bytes() > h->wide_stat_cap))
        return "place in the wide-symbol scratch outside it";
    if (p.S > kSeqMaxS && (p.S > r.wide_seq_S || !h->d_wide_symE || (size_t)r.n_wide_seq * r.wide_seq_S > h->wide_symE_cap))
        return "wide symbol without a row of symbolEnergy";
    if (cvt_format(p) >= 0 && (!r.cv || (const char *)p.in < r.cv->buf || (const char *)p.in + sizeof(float2) * p.n_in > r.cv->buf + r.cv->cap))
        return "converted CS16 / CS8 / CF16 packet outside the conversion scratch";
    return nullptr;
}
// PSK_SOFT_VALIDATE=1 (tests, the randomised comparison): what the kernels take for granted about a plan -- the samples a call reads
// exist, what it leaves behind fits the rings, its place in the scratch of the time-tiled kernels lies inside it -- is checked here, on the
// host, in front of the first launch; a violation refuses the call (nothing enqueued, nothing committed) instead of sending a kernel out of bounds.
psk_soft_status validate(const Round &r)
{
    for (uint32_t i = 0; i < r.nch; i++)
        if (const char *const why = r.plans[i].mode == psk::PLAN_SKIP ? nullptr : invalid_plan(r, r.plans[i])) {
            char buf[200];
            std::snprintf(buf, sizeof buf, "psk_soft_process: plan of channel %u fails validation: %s", r.ch0 + i, why);
            return fail(PSK_SOFT_ERR_LIMIT, buf);
        }
    return PSK_SOFT_OK;
}
// The schedule of the call: its window classes in launch order (deepest history first; class 0 stays on the caller's stream, the
// others take the side streams in turn), and whether they are joined at the end of the call, left on their streams (deferred) or
// -- *cut -- the call is handed back to be cut in time (nothing committed, nothing enqueued: the caller plans the pieces).
psk_soft_status choose_schedule(Round &r, bool *cut)
{
    psk_soft_handle *const h = r.h;
    const PlanSummary &res = r.res;
    for (int k = kNumClassH - 1; k >= 0; k--)
        for (int S : kFastS)
            if (res.cls[S][kClassH[k]].cnt)
                r.cls[r.n_cls++] = Cls{S, kClassH[k]};
    r.fork = r.n_cls > 1 && h->opt_fork;
    uint32_t listed = res.quiet.cnt, longest = 0;  // (listed != nch: channels without a packet this call, or on other launch sets)
    for (int i = 0; i < r.n_cls; i++) {
        const LaunchSet &s = res.cls[r.cls[i].S][r.cls[i].H];
        listed += s.cnt;
        longest = s.max_blocks > longest ? s.max_blocks : longest;
    }
    // only calls whose every channel runs on wave-scan launches are deferred or cut (nor calls with CS16 packets: the conversion
    // scratch is one per stream, and the next call's pre-pass must not overwrite it under the side streams of this one)
    const bool wave_scan_only = r.fork && !r.tile_syms && !res.any.cnt && !res.any_seq && !r.n_cvt && !r.n_wide_seq;
    r.deferred = wave_scan_only && (h->opt_deferred || r.of_split) && (!r.cont || r.of_split);
    if (wave_scan_only && !r.cont && !h->opt_deferred && h->opt_split > 1) {
        // Classes that cannot be resident together take two rounds of waves, and a wave that starts late still needs the whole call's
        // time at the lone-wave rate: cut in time, the late pieces are short too ("A mixed batch cut in time").
        static const uint32_t min_blocks = [] {  // (PSK_SOFT_SPLIT_MIN_BLOCKS: tests cut short calls too)
            const char *e = std::getenv("PSK_SOFT_SPLIT_MIN_BLOCKS");
            return e && std::atoi(e) > 0 ? (uint32_t)std::atoi(e) : kSplitMinBlocks;
        }();
        if (listed == r.nch && longest >= min_blocks) {
            *cut = true;
            return PSK_SOFT_OK;
        }
    }
    r.sig = 1469598103934665603ull;
    if (r.deferred) {
        auto mix = [&](uint64_t v) { r.sig = (r.sig ^ v) * 1099511628211ull; };
        mix(r.ch0), mix(r.nch), mix((uint64_t)(uintptr_t)r.stream), mix((uint64_t)r.n_cls), mix(res.quiet.cnt);
        for (int i = 0; i < r.n_cls; i++) mix(((uint64_t)r.cls[i].S << 40) | ((uint64_t)r.cls[i].H << 32) | res.cls[r.cls[i].S][r.cls[i].H].cnt);
        for (uint32_t i = 0; i < r.nch; i++) mix(r.h_list[i]);  // (no planned SKIP / SEQ channels here: the lists hold all nch)
        if (listed != r.nch)  // (channels without a packet this call: they belong to no stream -- the joined way)
            r.deferred = false;
    }
    if (h->deferred_pending && !(r.deferred && r.sig == h->deferred_sig)) {
        // a channel may be about to change streams: everything the side streams carry first
        // (its own earlier calls on another stream: wait_for_overlapping_calls has made this stream wait for them and their side streams)
        PSK_HIP(deferred_join(h, r.stream));
    }
    return PSK_SOFT_OK;
}
// header, plans, lists and whatever follows them of the call's slot, in one copy
psk_soft_status upload(Round &r)
{
    psk_soft_handle *const h = r.h;
    uint32_t *const hdr = psk::plan_header(h->h_plans[r.slot]);
    hdr[0] = 0u;                       // channels handed over: counted by the kernels
    hdr[1] = r.res.any_seq ? 1u : 0u;  // channels planned for the reference-order kernel
    const size_t up_bytes = (r.n_in_place || r.n_wide_seq) ? slot_seq_offset(r.nch) + sizeof(uint32_t) * r.nch
                            : r.n_cvt                      ? slot_cvt_offset(r.nch) + sizeof(psk::CvtDesc) * r.n_cvt
                                                           : psk::kPlanHeaderBytes + (sizeof(psk::ChanPlan) + sizeof(uint32_t)) * r.nch;
    if (h->opt_up_stream) {
        // (the slot's previous user has finished -- waited for in take_slot --, nothing else reads or writes d_plans[slot])
        PSK_HIP(hipMemcpyAsync(psk::plan_header(h->d_plans[r.slot]), hdr, up_bytes, hipMemcpyHostToDevice, h->up_stream));
        PSK_HIP(h->ev_up[r.slot].record(h->up_stream));
        PSK_HIP(h->ev_up[r.slot].wait(r.stream));
    } else {
        PSK_HIP(hipMemcpyAsync(psk::plan_header(h->d_plans[r.slot]), hdr, up_bytes, hipMemcpyHostToDevice, r.stream));
    }
    return PSK_SOFT_OK;
}
// phase ring of a launch: a power of two >= phaseAvg + 128 for its channels, at least 512 floats (256 where
// the energy ring is dynamic too and every byte of LDS counts towards residency)
inline uint32_t ring_floats(uint32_t n_max, uint32_t at_least)
{
    uint32_t y = at_least;
    while (y < n_max + 128u) y <<= 1;
    return y;
}
// (timing experiments only -- PSK_SOFT_DIAG_NO_TAIL=1: the exact-timing and reference-order launches behind the screened tier are
// left out, which is wrong as soon as a call is handed over; what the two launches cost a small call is measured that way)
bool diag_no_tail()
{
    static const bool on = std::getenv("PSK_SOFT_DIAG_NO_TAIL") && std::atoi(std::getenv("PSK_SOFT_DIAG_NO_TAIL")) != 0;
    return on;
}
// PSK_SOFT_TRACE_LAUNCHES=1 (debugging a faulting kernel): in front of every launch the host waits for everything enqueued so far and
// writes one line for the launch and one per channel of its list to stderr -- the last launch named in the log of a run that died is the
// one that did it, with the shapes it was given.  (=2: the launch lines only.)  trace_launch: the launch line, of every launch of the
// library -- the rounds' (mark), the quality pass's, the gathers', the acquire pass's.
hipError_t trace_launch(const psk_soft_handle *h, const char *what, int S, int H, uint32_t ch0, uint32_t cnt, uint64_t tiles, uint32_t y_len,
                        uint32_t r_len, int slot, hipStream_t stream)
{
    if (!h->opt_trace)
        return hipSuccess;
    if (const hipError_t e = hipDeviceSynchronize())
        return e;
    std::fprintf(stderr, "[psk_soft] ok; next: %s S=%d H=%d ch0=%u cnt=%u tiles=%llu y_len=%u r_len=%u slot=%d stream=%p\n", what, S, H, ch0, cnt,
                 (unsigned long long)tiles, y_len, r_len, slot, (void *)stream);
    std::fflush(stderr);
    return hipSuccess;
}
// ... of a round's launch, and the channel lines behind it.  off: the launch's place in the lists; ~0u: the whole batch.
hipError_t mark(const Round &r, hipStream_t st, const char *what, int S, int H, uint32_t off, uint32_t cnt, uint32_t tiles, uint32_t y_len,
                uint32_t r_len)
{
    const hipError_t e = trace_launch(r.h, what, S, H, r.ch0, cnt, tiles, y_len, r_len, r.slot, st);
    if (e != hipSuccess || r.h->opt_trace != 1)
        return e;
    for (uint32_t i = 0; i < cnt; i++) {
        const uint32_t bi = r.stamped || off == ~0u ? i : r.h_list[off + i];
        const psk::ChanPlan &p = r.plans[bi];
        if (off == ~0u && p.mode == psk::PLAN_SKIP)
            continue;
        std::fprintf(stderr, "[psk_soft]   ch %u mode=%u S=%u A=%u M=%u n=%u len0=%u n_out=%llu n_in=%llu L0=%u L1=%u flags=0x%x K=%u tbase=%u toff=%llu in=%p\n",
                     r.ch0 + bi, p.mode, p.S, p.A, p.M, p.lf_n, p.lf_len0, (unsigned long long)p.n_out, (unsigned long long)p.n_in, p.ring_len0,
                     p.ring_len1, p.lf_flags, p.tile_blocks, p.tile_base, (unsigned long long)p.tile_off, (const void *)p.in);
    }
    std::fflush(stderr);
    return hipSuccess;
}
// What tells the time-tiled launch sets apart: the front stage (of a window class, of the sets without an instantiation, of the wide
// symbols: psk_wide.hip), the fit stage (window in LDS, or the far fit's in device memory) and how their launches are traced: names, and S, H,
// y_len and r_len as the lines give them (r_front: of the front stage's line -- wide_z for the wide symbols; the parallel fit's has pf_second there)
enum class Front { window_class, any, wide };
enum class Fit { lds, far };
struct TiledTrace {
    const char *front, *pfit, *fit, *back;
    int S, H;
    uint32_t y_len, r_front, r_len;
};
// The chain of a time-tiled set that is not pipelined: front stage (screened timing and picks into the scratch), fit stage, back
// stage (the outputs).  (A call these cannot carry comes out with guard 1 and nothing committed: the launches behind them redo it.)
psk_soft_status enqueue_tiled(const Round &r, const LaunchSet &s, const TiledTrace &t, Front front, Fit fit, hipStream_t st)
{
    psk_soft_handle *const h = r.h;
    const uint32_t *const l = r.d_list + s.off;
    const uint32_t ring_cap = h->lim.ring_cap, fit_cap = h->lim.fit_cap;
    PSK_HIP(mark(r, st, t.front, t.S, t.H, s.off, s.cnt, s.tiles_max, t.y_len, t.r_front));
    if (front == Front::window_class)
        PSK_HIP(psk::launch_tile_front(t.S, class_H(t.H), r.d_plans, l, r.ch0, s.cnt, s.tiles_max, h->d_state, h->d_ring, ring_cap, t.r_len, h->d_tiles,
                                       h->d_traw, h->d_ts, h->pf.chan, 0u, st));
    else if (front == Front::any)
        PSK_HIP(psk::launch_tile_front_any(r.d_plans, l, r.ch0, s.cnt, s.tiles_max, s.max_S, h->d_state, h->d_ring, ring_cap, h->d_tiles, h->d_traw,
                                           h->d_ts, h->pf.chan, st));
    else
        PSK_HIP(psk::launch_wide_front(r.d_plans, l, r.ch0, s.cnt, s.tiles_max, s.max_S, h->d_ring, ring_cap, h->d_tiles, h->d_traw, h->d_ts,
                                       h->pf.chan, h->d_wide_rec, h->d_wide_stat, st));
    if (fit == Fit::lds && h->opt_pfit) {  // (the parallel fit, then the block-by-block fit for what it leaves)
        PSK_HIP(mark(r, st, t.pfit, t.S, t.H, s.off, s.cnt, s.tiles_max, t.y_len, r.pf_second));
        PSK_HIP(psk::launch_pfit(r.d_plans, l, r.ch0, s.cnt, s.tiles_max, h->d_state, h->d_ring, ring_cap, h->d_yv, fit_cap, t.y_len, h->d_tiles,
                                 h->d_traw, h->d_ts, h->d_test, h->pf, r.pf_second, st));
    }
    PSK_HIP(mark(r, st, t.fit, t.S, t.H, s.off, s.cnt, s.tiles_max, t.y_len, t.r_len));
    if (fit == Fit::lds)
        PSK_HIP(psk::launch_tile_fit(r.d_plans, l, r.ch0, s.cnt, h->d_state, h->d_ring, ring_cap, h->d_yv, fit_cap, t.y_len, h->d_tiles, h->d_traw,
                                     h->d_ts, h->d_test, h->pf, st));
    else
        PSK_HIP(psk::launch_far_fit(r.d_plans, l, r.ch0, s.cnt, h->d_state, h->d_ring, ring_cap, h->d_yv, fit_cap, h->d_far_y, h->far_rows_cap,
                                    h->d_tiles, h->d_traw, h->d_ts, h->d_test, st));
    PSK_HIP(mark(r, st, t.back, t.S, t.H, s.off, s.cnt, s.tiles_max, t.y_len, t.r_len));
    PSK_HIP(psk::launch_tile_back(r.d_plans, l, r.ch0, s.cnt, s.tiles_max, h->d_state, h->d_tiles, h->d_ts, h->d_test, 0u, 0u, st));
    return PSK_SOFT_OK;
}
// the sets without an instantiation on the caller's stream: any, wide, then the far fit's quiet calls and its two sets -- the same
// front and back stages around the fit stage with its rings in device memory (no LDS ring: y_len 0)
psk_soft_status enqueue_any_sets(const Round &r)
{
    psk_soft_handle *const h = r.h;
    const PlanSummary &res = r.res;
    const LaunchSet &any = res.any, &wide = res.wide, &anyf = res.anyf, &widef = res.widef;
    if (any.cnt)
        PSK_TRY(enqueue_tiled(r, any, {"tile_front_any", "pfit (any)", "tile_fit (any)", "tile_back (any)", any.max_S, 0, ring_floats(any.max_n, 512u), 0, 0},
                              Front::any, Fit::lds, r.stream));
    if (wide.cnt)
        PSK_TRY(enqueue_tiled(r, wide, {"wide_front (chunk, pick)", "pfit (wide)", "tile_fit (wide)", "tile_back (wide)", wide.max_S, 0,
                                        ring_floats(wide.max_n, 512u), r.wide_z, 0},
                              Front::wide, Fit::lds, r.stream));
    if (res.quietf.cnt) {
        PSK_HIP(mark(r, r.stream, "far_quiet (calls that emit nothing)", 0, 0, res.quietf.off, res.quietf.cnt, 0, 0, 0));
        PSK_HIP(psk::launch_far_quiet(h->d_plans[r.slot], r.d_list + res.quietf.off, r.ch0, res.quietf.cnt, h->d_state, h->d_ring, h->lim.ring_cap,
                                      h->d_yv, h->lim.fit_cap, h->d_far_y, h->far_rows_cap, r.stream));
    }
    if (anyf.cnt)
        PSK_TRY(enqueue_tiled(r, anyf, {"tile_front_any (far)", nullptr, "far_fit (any)", "tile_back (any, far)", anyf.max_S, 0, 0, 0, 0}, Front::any,
                              Fit::far, r.stream));
    if (widef.cnt)
        PSK_TRY(enqueue_tiled(r, widef, {"wide_front (chunk, pick; far)", nullptr, "far_fit (wide)", "tile_back (wide, far)", widef.max_S, 0, 0, r.wide_z, 0},
                              Front::wide, Fit::far, r.stream));
    return PSK_SOFT_OK;
}
// A pipelined class: front(range j) on the class's stream, fit(range j) on a second stream behind it -- under front(range j + 1) --,
// back(range j) on a third behind that (psk_tile.hip: psk_tile_fit_range_kernel)
psk_soft_status enqueue_piped(const Round &r, const LaunchSet &s, int S, int H, uint32_t y_len, uint32_t r_len, hipStream_t st)
{
    psk_soft_handle *const h = r.h;
    const uint32_t cnt = s.cnt, T = s.tiles_max, tr = s.pipe_tiles;
    const uint32_t *const l = r.d_list + s.off;
    char *const carry = static_cast<char *>(h->d_pipe_carry) + psk::pipe_carry_bytes() * s.off;
    float *const carry_y = h->d_pipe_y + (size_t)kPipeMaxYLen * s.off;
    const uint32_t y_pipe = ring_floats(s.max_n, 512u);
    int e = 0;
    PSK_HIP(h->pipe_ev[e].record(st));  // (the side streams start behind everything this one carries)
    PSK_HIP(h->pipe_ev[e].wait(h->pipe_st[0]));
    PSK_HIP(h->pipe_ev[e].wait(h->pipe_st[1]));
    e++;
    for (uint32_t t0 = 0; t0 < T; t0 += tr) {
        const uint32_t nt = T - t0 < tr ? T - t0 : tr;
        PSK_HIP(mark(r, st, "pipe_front", S, H, s.off, cnt, nt, y_len, r_len));
        PSK_HIP(psk::launch_tile_front(S, class_H(H), r.d_plans, l, r.ch0, cnt, nt, h->d_state, h->d_ring, h->lim.ring_cap, r_len, h->d_tiles,
                                       h->d_traw, h->d_ts, h->pf.chan, t0, st));
        PSK_HIP(h->pipe_ev[e].record(st));
        PSK_HIP(h->pipe_ev[e].wait(h->pipe_st[0]));
        e++;
        PSK_HIP(mark(r, h->pipe_st[0], "pipe_fit", S, H, s.off, cnt, nt, y_pipe, 0));
        PSK_HIP(psk::launch_tile_fit_range(r.d_plans, l, r.ch0, cnt, h->d_state, h->d_ring, h->lim.ring_cap, h->d_yv, h->lim.fit_cap, y_pipe,
                                           h->d_tiles, h->d_traw, h->d_ts, h->d_test, carry, carry_y, t0, nt, h->pipe_st[0]));
        PSK_HIP(h->pipe_ev[e].record(h->pipe_st[0]));
        PSK_HIP(h->pipe_ev[e].wait(h->pipe_st[1]));
        e++;
        PSK_HIP(mark(r, h->pipe_st[1], "pipe_back", S, H, s.off, cnt, nt, y_pipe, 0));
        PSK_HIP(psk::launch_tile_back(r.d_plans, l, r.ch0, cnt, nt, h->d_state, h->d_tiles, h->d_ts, h->d_test, t0, 1u, h->pipe_st[1]));
    }
    PSK_HIP(h->pipe_ev[e].record(h->pipe_st[1]));  // (behind the last fit too: the last back waited for it)
    PSK_HIP(h->pipe_ev[e].wait(st));
    return PSK_SOFT_OK;
}
// One window class (samplesPerBaud, history depth) on its stream: the time-tiled kernels first where it has its tiles; then screened
// timing, then the exact-timing instantiation, which picks up the calls the screening refused (the reference-order kernel: those of both).
psk_soft_status enqueue_class(const Round &r, int S, int H, hipStream_t st)
{
    psk_soft_handle *const h = r.h;
    const LaunchSet &s = r.res.cls[S][H];
    const uint32_t *const l = r.d_list + s.off;
    const uint32_t y_len = ring_floats(s.max_n, psk::ering_dynamic(S) ? 256u : 512u);
    const uint32_t r_len = class_H(H) == 1 ? ((s.max_A + 128u + 1u) & ~1u) : 0u;
    if (s.tiled && s.piped)
        PSK_TRY(enqueue_piped(r, s, S, H, y_len, r_len, st));
    else if (s.tiled)
        PSK_TRY(enqueue_tiled(r, s, {"tile_front", "pfit", "tile_fit", "tile_back", S, H, y_len, r_len, r_len}, Front::window_class, Fit::lds, st));
    // (the exact tier only works on the calls the tier in front of it left; behind the time-tiled kernels, whose front
    // stage IS the screened timing, it is the exact tier that picks up what they hand over)
    const psk::PktFormat *const f = class_pkt(H);
    for (int exact = s.tiled ? 1 : 0; exact <= 1; exact++) {
        if (exact && diag_no_tail())
            break;
        PSK_HIP(mark(r, st, exact ? "fast (exact tier)" : "fast (screened tier)", S, H, s.off, s.cnt, 0, y_len, r_len));
        if (f)
            PSK_HIP(psk::launch_fast_pkt((int)f->id, S, exact, r.d_plans, l, r.ch0, s.cnt, h->d_state, h->d_ring, h->lim.ring_cap, h->d_yv,
                                         h->lim.fit_cap, y_len, r_len, st));
        else
            PSK_HIP(psk::launch_fast(S, class_H(H), exact, r.d_plans, l, r.ch0, s.cnt, h->d_state, h->d_ring, h->lim.ring_cap, h->d_yv,
                                     h->lim.fit_cap, y_len, r_len, st));
    }
    if (r.deferred && f)  // (the class's hand-overs are redone on its own stream, in front of its next call)
        PSK_HIP(psk::launch_seq_pkt((int)f->id, r.d_plans, l, r.ch0, s.cnt, h->d_state, h->d_ring, h->lim.ring_cap, h->d_yv, h->lim.fit_cap, st));
    else if (r.deferred)
        PSK_HIP(psk::launch_seq(r.d_plans, l, r.ch0, s.cnt, h->d_state, h->d_ring, h->lim.ring_cap, h->d_yv, h->lim.fit_cap, st));
    return PSK_SOFT_OK;
}
// The end of the call: deferred, the side streams keep what they carry (an event each, for the slot); joined, the caller's stream waits for
// them and the reference-order kernel takes the calls planned for it or handed over -- each of its builds on its own channels.
psk_soft_status enqueue_join_and_tail(Round &r, int used_aux)
{
    psk_soft_handle *const h = r.h;
    const hipStream_t st = r.stream;
    if (r.deferred) {
        for (int a = 0; a < used_aux && a < kAuxStreams; a++) PSK_HIP(h->slot_aux_ev[r.slot][a].record(h->aux[a]));  // (created here)
        h->deferred_pending = true, h->deferred_sig = r.sig, h->deferred_stream = st;
        return PSK_SOFT_OK;
    }
    for (int a = 0; a < used_aux && a < kAuxStreams; a++) {
        PSK_HIP(h->aux_join[a].record(h->aux[a]));
        PSK_HIP(h->aux_join[a].wait(st));
    }
    if (!r.res.any_seq && !r.res.any_emit)  // (any_emit: the exactness guard may hand calls over at run time)
        return PSK_SOFT_OK;
    PSK_HIP(mark(r, st, "seq (reference order)", 0, 0, ~0u, r.nch, 0, 0, 0));
    if (diag_no_tail())
        return PSK_SOFT_OK;
    if (!r.n_in_place && !r.n_wide_seq) {
        PSK_HIP(psk::launch_seq(r.d_plans, nullptr, r.ch0, r.nch, h->d_state, h->d_ring, h->lim.ring_cap, h->d_yv, h->lim.fit_cap, st));
        return PSK_SOFT_OK;
    }
    const uint32_t *const d_seq =
        reinterpret_cast<const uint32_t *>(reinterpret_cast<const char *>(psk::plan_header(r.d_plans)) + slot_seq_offset(r.nch));
    PSK_HIP(psk::launch_seq(r.d_plans, d_seq, r.ch0, r.n_seq_narrow, h->d_state, h->d_ring, h->lim.ring_cap, h->d_yv, h->lim.fit_cap, st));
    const uint32_t *d_seq_f = d_seq + r.n_seq_narrow;
    for (int f = 0; f < psk::kNumPktFormats; d_seq_f += r.n_in_place_f[f], f++)
        PSK_HIP(psk::launch_seq_pkt((int)psk::kPktFormats[f].id, r.d_plans, d_seq_f, r.ch0, r.n_in_place_f[f], h->d_state, h->d_ring, h->lim.ring_cap,
                                    h->d_yv, h->lim.fit_cap, st));
    if (r.n_wide_seq)
        PSK_HIP(mark(r, st, "seq_wide (reference order, samplesPerBaud > 1024)", (int)r.wide_seq_S, 0, ~0u, 0, 0, 0, 0));
    PSK_HIP(psk::launch_seq_wide(r.d_plans, d_seq + (r.nch - r.n_wide_seq), r.ch0, r.n_wide_seq, h->d_state, h->d_ring, h->lim.ring_cap, h->d_yv,
                                 h->lim.fit_cap, h->d_wide_symE, r.wide_seq_S, st));
    return PSK_SOFT_OK;
}
// Every launch of the call, in order: conversion pre-passes, the channels that emit nothing, the sets without an instantiation, then
// the window classes.  A batch that mixes classes runs them SIDE BY SIDE -- each class is its own instantiation with its own register
// and LDS appetite, and one after the other each would leave part of the machine idle --: on side streams forked off the caller's
// behind the plan upload and joined again in front of the reference-order kernel; the deepest histories are launched first.
psk_soft_status enqueue(Round &r)
{
    psk_soft_handle *const h = r.h;
    const PlanSummary &res = r.res;
    const hipStream_t stream = r.stream;
    const psk::CvtDesc *d_desc = reinterpret_cast<const psk::CvtDesc *>(reinterpret_cast<const char *>(psk::plan_header(r.d_plans)) + slot_cvt_offset(r.nch));
    for (int f = 0; f < psk::kNumPktFormats; d_desc += r.n_cvt_f[f], f++) {
        if (!r.n_cvt_f[f])
            continue;
        PSK_HIP(mark(r, stream, psk::kPktFormats[f].convert, 0, 0, ~0u, 0, r.n_cvt_f[f], 0, 0));
        PSK_HIP(psk::launch_convert((int)psk::kPktFormats[f].id, d_desc, r.n_cvt_f[f], r.cvt_max_n[f], stream));
    }
    if (res.quiet.cnt) {
        const uint32_t y_len = ring_floats(res.quiet.max_n, 512u);
        PSK_HIP(mark(r, stream, "fast<0,1> (calls that emit nothing)", 0, 1, res.quiet.off, res.quiet.cnt, 0, y_len, 0));
        PSK_HIP(psk::launch_fast(0, 1, 0, r.d_plans, r.d_list + res.quiet.off, r.ch0, res.quiet.cnt, h->d_state, h->d_ring, h->lim.ring_cap, h->d_yv,
                                 h->lim.fit_cap, y_len, 0u, stream));
    }
    PSK_TRY(enqueue_any_sets(r));
    if (res.quiet.cnt && r.deferred)  // (every launch set ends its own calls: the quiet channels' on the caller's stream)
        PSK_HIP(psk::launch_seq(r.d_plans, r.d_list + res.quiet.off, r.ch0, res.quiet.cnt, h->d_state, h->d_ring, h->lim.ring_cap, h->d_yv,
                                h->lim.fit_cap, stream));
    if (r.fork) {
        if (!h->aux_fork) {  // (the side streams, created at the first call that mixes window classes)
            PSK_HIP(h->aux_fork.ensure());
            // (streams of one priority share a few hardware queues, and two streams that land on the same one run their kernels one
            // after the other: a stream of another priority gets a queue of its own -- DESIGN.md 3.5)
            int prio_lo = 0, prio_hi = 0;
            PSK_HIP(hipDeviceGetStreamPriorityRange(&prio_lo, &prio_hi));
            for (int k = 0; k < kAuxStreams; k++) {
                const char *pe = getenv("PSK_SOFT_AUX_PRIO");
                const int mode = pe ? atoi(pe) : 1;
                if (mode == 0 || prio_lo == prio_hi)
                    PSK_HIP(h->aux[k].create());
                else
                    PSK_HIP(h->aux[k].create(mode == 1 ? prio_hi : prio_lo));
                PSK_HIP(h->aux_join[k].ensure());
            }
        }
        PSK_HIP(h->aux_fork.record(stream));
    }
    int used_aux = 0;
    for (int i = 0; i < r.n_cls; i++) {
        // class 0 stays on the caller's stream, the others take the side streams in turn
        hipStream_t st = stream;
        if (r.fork && i > 0) {
            const int a = (i - 1) % kAuxStreams;
            st = h->aux[a];
            if (i - 1 < kAuxStreams) {
                PSK_HIP(h->aux_fork.wait(st));
                used_aux = i;
            }
        }
        PSK_TRY(enqueue_class(r, r.cls[i].S, r.cls[i].H, st));
    }
    PSK_TRY(enqueue_join_and_tail(r, used_aux));
    if (r.tile_syms || r.n_wide_seq)
        PSK_HIP(h->tile_ev.record(stream));
    if (r.n_cvt)
        PSK_HIP(r.cv->ev.record(stream));
    PSK_HIP(h->ev[r.slot].record(stream));
    return PSK_SOFT_OK;
}
// What a round is of: the whole call (cont == nullptr), or a piece of a call the library has cut (process_device_call) -- cont[i]: bit 0 =
// packet i continues the call of the packet before it (plan_call's `cont`), bit 1 = more pieces of the call follow (no end-of-call wrap
// yet), bit 2 = the piece is cut where the reference does not rebuild its sums.  of_split: the pieces are those of a mixed batch cut in time.
struct Pieces {
    const uint8_t *cont = nullptr;
    bool of_split = false;
};
// What process_round decided about a whole call, next to its status: enqueued (or nothing to do); some channel's call is too long for one
// piece -- the caller cuts it at the resync boundaries --; or the batch mixes window classes that cannot be resident together -- the caller
// cuts every channel's call into `pieces` pieces in time and lets the classes run through them on their own streams, joined once at the
// end of the call (process_device_call).  With the last two nothing is committed and nothing enqueued.
struct Verdict {
    enum { done, too_long, mixed } what = done;
    int pieces = 0;
};
// One pass of the control plane over a batch and the launches it asks for, phase by phase.
psk_soft_status process_round(psk_soft_handle_t *h, uint32_t ch0, uint32_t nch, const psk_soft_packet_t *pkts, psk_soft_output_t *outs,
                              void *stream_v, const Pieces &pieces, Verdict *verdict)
{
    const uint8_t *const cont = pieces.cont;
    *verdict = Verdict{};
    if (!h || !pkts || !outs || !nch || (uint64_t)ch0 + nch > h->nch)
        return fail(PSK_SOFT_ERR_INVALID_ARG, "psk_soft_process: bad arguments");
    if (h->poisoned)
        return fail(PSK_SOFT_ERR_HIP, "psk_soft_process: an earlier call failed inside HIP after its kernels were enqueued; the "
                                      "channel states are undefined -- destroy the handle (or import saved states into a new one)");
    Round r{h, ch0, nch, pkts, outs, cont, pieces.of_split, stream_v ? (hipStream_t)stream_v : h->stream, h->slot, h->dry,
            (h->opt_qpsk_sign_map ? (uint32_t)psk::PLAN_QPSK_SIGN_MAP : 0u) | (h->opt_ties_in_place ? 0u : (uint32_t)psk::PLAN_TIES_HANDOVER), h->lim};
    PSK_TRY(take_slot(r));
    plan_stamped(r);
    if (!r.stamped) {
        ctl_touch_range(h, ch0, ch0 + nch);  // (the ordinary path writes the channels one by one)
        plan_each(r);
    }
    if (r.res.st == PSK_SOFT_OK && r.res.long_call && !cont) {
        verdict->what = Verdict::too_long;
        return PSK_SOFT_OK;
    }
    if (r.res.st != PSK_SOFT_OK)
        return refusal(r);
    if (h->dry || !r.res.any_plan) {
        commit(r);
        return PSK_SOFT_OK;
    }
    PSK_TRY(wait_for_overlapping_calls(r));
    // lists and places, then the scratch they need: every phase may send channels to the reference-order kernel instead
    move_in_place_back(r);
    fill_lists(r);
    place_all(r);
    for (psk_soft_status (*phase)(Round &) : {scratch_tiles, scratch_wide, scratch_far_rows, scratch_wide_seq, scratch_order, conversion_descriptors})
        PSK_TRY(phase(r));
    reference_order_lists(r);
    if (h->opt_validate)
        PSK_TRY(validate(r));
    bool cut = false;
    PSK_TRY(choose_schedule(r, &cut));
    if (cut) {
        *verdict = Verdict{Verdict::mixed, h->opt_split};
        return PSK_SOFT_OK;
    }
    PSK_TRY(upload(r));
    const psk_soft_status est = enqueue(r);
    if (est != PSK_SOFT_OK) {
        h->poisoned = true;
        return est;
    }
    commit(r);
    if (r.tile_syms || r.n_wide_seq)
        h->tile_stream = r.stream;
    h->slot = (h->slot + 1) % kPlanSlots;
    h->slot_stream[r.slot] = r.stream, h->slot_ch0[r.slot] = ch0, h->slot_nch[r.slot] = nch;
    return PSK_SOFT_OK;
}

// The tail of every psk_soft_get_* of the reduction-pass layer: records [first, first + n) of an entry whose arguments have passed,
// once every call and every pass of its ring enqueued so far has ended.
template <class Rec, class Ring>
psk_soft_status records_read(psk_soft_handle_t *h, const Records<Rec> &recs, Ring &ring, uint32_t first, uint32_t n, Rec *out)
{
    if (h->dry) {
        std::memcpy(out, recs.dry.data() + first, sizeof(Rec) * n);
        return PSK_SOFT_OK;
    }
    PSK_TRY(psk_soft_synchronize(h));
    PSK_TRY(ring.wait());
    PSK_HIP(hipMemcpy(out, recs.d + first, sizeof(Rec) * n, hipMemcpyDeviceToHost));
    return PSK_SOFT_OK;
}
}  // namespace

extern "C" {

uint32_t psk_soft_abi_version(void) { return PSK_SOFT_ABI_VERSION; }
const char *psk_soft_last_error(void) { return g_last_error.c_str(); }

psk_soft_status psk_soft_create(int device, uint32_t n_channels, const psk_soft_limits_t *limits,
                                psk_soft_handle_t **out)
{
    if (!out || !n_channels)
        return fail(PSK_SOFT_ERR_INVALID_ARG, "psk_soft_create: null output or zero channels");
    *out = nullptr;
    psk_soft_limits_t lim;
    lim.max_window_samples = 16384;
    lim.max_phase_avg = 512;
    lim.max_packet_complex = 1u << 20;
    if (limits)
        lim = *limits;
    if (lim.max_window_samples < 16 || lim.max_phase_avg < 1)
        return fail(PSK_SOFT_ERR_INVALID_ARG, "psk_soft_create: limits too small");
    psk_soft_handle *h = new (std::nothrow) psk_soft_handle();
    if (!h)
        return fail(PSK_SOFT_ERR_INVALID_ARG, "out of host memory");
    h->nch = n_channels;
    h->user = lim;
    h->lim.ring_cap = lim.max_window_samples;
    h->lim.fit_cap = lim.max_phase_avg + 1;  // circular yvals buffer
    h->lim.fast_fit_max = kFastFitMax;
    h->lim.force_seq = false;
    h->lim.far_fit = false;
    h->ctl.resize(n_channels);
    h->ctl_next.resize(n_channels);
    h->last_mode.assign(n_channels, psk::PLAN_SKIP);
    h->dry = (device == PSK_SOFT_DEVICE_NONE);  // (h->device: set below, once the device has been found usable)
    if (const char *e = std::getenv("PSK_SOFT_TIME_TILED"))
        h->opt_tiled = std::atoi(e) < 0 ? 0 : std::atoi(e) > 2 ? 2 : std::atoi(e);
    if (const char *e = std::getenv("PSK_SOFT_FAR_FIT"))  // (as psk_soft_set_option(PSK_SOFT_OPT_FAR_FIT))
        h->opt_far_fit = std::atoi(e) != 0;
    h->lim.far_fit = h->opt_far_fit != 0;
    if (const char *e = std::getenv("PSK_SOFT_TIES_IN_PLACE"))
        h->opt_ties_in_place = std::atoi(e) != 0;
    if (const char *e = std::getenv("PSK_SOFT_TRACE_LAUNCHES"))
        h->opt_trace = std::atoi(e);
    if (const char *e = std::getenv("PSK_SOFT_VALIDATE"))
        h->opt_validate = std::atoi(e);
    if (const char *e = std::getenv("PSK_SOFT_DIAG_GATHER_ONLY"))
        h->opt_diag_gather_only = std::atoi(e) != 0;
    if (const char *e = std::getenv("PSK_SOFT_SPLIT_CLASSES"))
        h->opt_split = std::atoi(e) < 0 ? 0 : std::atoi(e) > 16 ? 16 : std::atoi(e);
    if (const char *e = std::getenv("PSK_SOFT_PIPELINED"))
        h->opt_pipe = std::atoi(e) < 0 ? 0 : std::atoi(e) > 2 ? 2 : std::atoi(e);
    if (const char *e = std::getenv("PSK_SOFT_DEFERRED_JOIN"))  // (as psk_soft_set_option(PSK_SOFT_OPT_DEFERRED_JOIN))
        h->opt_deferred = std::atoi(e) != 0;
    if (const char *e = std::getenv("PSK_SOFT_STAMP"))
        h->opt_stamp = std::atoi(e) != 0;
    if (const char *e = std::getenv("PSK_SOFT_PARALLEL_FIT"))
        h->opt_pfit = std::atoi(e) < 0 ? 0 : std::atoi(e) > 2 ? 2 : std::atoi(e);
    // the one way out of a create that fails: the handle goes the way every handle goes, whatever it holds by then
    auto bail = [&](psk_soft_status st, const std::string &msg) {
        const std::string keep = msg;
        psk_soft_destroy(h);
        return fail(st, keep);
    };
    auto bail_hip = [&](const char *what, hipError_t e2) {
        return bail(PSK_SOFT_ERR_HIP, std::string("psk_soft_create: ") + what + ": " + hipGetErrorString(e2));
    };
    if (!h->dry) {
        int ndev = 0;
        hipError_t e = hipGetDeviceCount(&ndev);
        if (e != hipSuccess || ndev <= 0 || device < 0 || device >= ndev)
            return bail(PSK_SOFT_ERR_NO_DEVICE, std::string("psk_soft_create: no usable HIP device (") +
                                                    (e != hipSuccess ? hipGetErrorString(e) : "device index out of range") + ")");
        hipDeviceProp_t prop;
        if (hipSetDevice(device) != hipSuccess || hipGetDeviceProperties(&prop, device) != hipSuccess)
            return bail(PSK_SOFT_ERR_NO_DEVICE, "psk_soft_create: hipSetDevice failed");
        if (std::strncmp(prop.gcnArchName, "gfx950", 6) != 0)
            return bail(PSK_SOFT_ERR_NO_DEVICE, std::string("psk_soft_create: kernels are built for gfx950 only, device is ") + prop.gcnArchName);
        h->device = device;
        hipError_t e2;
        if ((e2 = h->stream.create()) != hipSuccess)
            return bail_hip("hipStreamCreate", e2);
        size_t state_b = sizeof(psk::ChanState) * (size_t)n_channels;
        size_t ring_b = sizeof(float2) * 2u * (size_t)h->lim.ring_cap * n_channels;
        size_t yv_b = sizeof(float) * (size_t)h->lim.fit_cap * n_channels;
        if ((e2 = h->d_state.alloc_bytes(state_b)) != hipSuccess) return bail_hip("hipMalloc state", e2);
        if ((e2 = h->d_ring.alloc_bytes(ring_b)) != hipSuccess) return bail_hip("hipMalloc ring", e2);
        if ((e2 = h->d_yv.alloc_bytes(yv_b)) != hipSuccess) return bail_hip("hipMalloc yvals", e2);
        // psk_soft_i constructor state: phaseEstimate 0, last (0,0), LinearFit denominator 1, xAvg 0
        // (cpp/psk_soft.cpp:35-46, 187-199)
        std::vector<psk::ChanState> init(n_channels);
        std::memset(init.data(), 0, state_b);
        for (auto &s : init) s.lf_den = 1.0f;
        if ((e2 = hipMemcpy(h->d_state, init.data(), state_b, hipMemcpyHostToDevice)) != hipSuccess)
            return bail_hip("hipMemcpy state", e2);
        if ((e2 = hipMemset(h->d_ring, 0, ring_b)) != hipSuccess) return bail_hip("hipMemset", e2);
        if ((e2 = hipMemset(h->d_yv, 0, yv_b)) != hipSuccess) return bail_hip("hipMemset", e2);
        for (int s = 0; s < kPlanSlots; s++) {
            // (a slot = the plans of a call followed by the compact channel lists of its launches: one upload)
            // (... behind the header the kernels find in front of the plans: psk_plan.h)
            if ((e2 = h->h_plan_blk[s].alloc(slot_bytes(n_channels))) != hipSuccess)
                return bail_hip("hipHostMalloc plans", e2);
            std::memset(h->h_plan_blk[s], 0, psk::kPlanHeaderBytes);
            h->h_plans[s] = reinterpret_cast<psk::ChanPlan *>(h->h_plan_blk[s] + psk::kPlanHeaderBytes);
            if ((e2 = h->d_plan_blk[s].alloc(slot_bytes(n_channels))) != hipSuccess)
                return bail_hip("hipMalloc plans", e2);
            h->d_plans[s] = reinterpret_cast<psk::ChanPlan *>(h->d_plan_blk[s] + psk::kPlanHeaderBytes);
            if ((e2 = h->ev[s].ensure()) != hipSuccess)
                return bail_hip("hipEventCreate", e2);
            if ((e2 = h->ev_up[s].ensure()) != hipSuccess)
                return bail_hip("hipEventCreate", e2);
        }
        if ((e2 = h->up_stream.create()) != hipSuccess)
            return bail_hip("hipStreamCreate", e2);
        if (const char *e = std::getenv("PSK_SOFT_PLAN_STREAM"))
            h->opt_up_stream = std::atoi(e) != 0;
    }
    // the records of the quality pass and of the two looks: zeros until a pass writes one (the word search's come with its first call)
    if (h->quality.ensure_zeroed(h->dry, n_channels, "psk_soft_create: quality records") != PSK_SOFT_OK ||
        h->acquire.ensure_zeroed(h->dry, n_channels, "psk_soft_create: acquire records") != PSK_SOFT_OK ||
        h->symrate.ensure_zeroed(h->dry, n_channels, "psk_soft_create: symrate records") != PSK_SOFT_OK)
        return bail(PSK_SOFT_ERR_HIP, g_last_error);
    *out = h;
    return PSK_SOFT_OK;
}

psk_soft_status psk_soft_destroy(psk_soft_handle_t *h)
{
    if (!h)
        return PSK_SOFT_OK;
    // Every stream the handle owns is idle before anything is released (an absent stream: no HIP call); the members' destructors do
    // the rest, in whatever order.
    if (h->device != PSK_SOFT_DEVICE_NONE)
        (void)hipSetDevice(h->device);
    (void)h->stream.sync(), (void)h->up_stream.sync();
    for (const Stream &s : h->aux) (void)s.sync();
    for (const Stream &s : h->pipe_st) (void)s.sync();
    for (const StageSlot &sl : h->stage) (void)sl.stream.sync();
    delete h;
    return PSK_SOFT_OK;
}

psk_soft_status psk_soft_configure(psk_soft_handle_t *h, uint32_t ch0, uint32_t nch, const psk_soft_props_t *props)
{
    if (!h || !props || (uint64_t)ch0 + nch > h->nch)
        return fail(PSK_SOFT_ERR_INVALID_ARG, "psk_soft_configure: bad channel range");
    for (uint32_t i = 0; i < nch; i++) {
        const psk_soft_props_t &p = props[i];
        if ((uint64_t)p.samplesPerBaud * p.numAvg > h->lim.ring_cap || p.phaseAvg >= h->lim.fit_cap)
            return fail(PSK_SOFT_ERR_LIMIT, "psk_soft_configure: property exceeds the limits given at create "
                                            "(samplesPerBaud*numAvg, phaseAvg)");
    }
    ctl_touch(h);
    for (uint32_t i = 0; i < nch; i++) h->ctl[ch0 + i].configure(props[i]);
    return PSK_SOFT_OK;
}

psk_soft_status psk_soft_query(const psk_soft_handle_t *h, uint32_t ch, psk_soft_props_t *props)
{
    if (!h || !props || ch >= h->nch)
        return fail(PSK_SOFT_ERR_INVALID_ARG, "psk_soft_query: bad channel");
    ctl_sync(h);
    *props = h->ctl[ch].props;
    return PSK_SOFT_OK;
}

psk_soft_status psk_soft_fire_listener(psk_soft_handle_t *h, uint32_t ch, int which)
{
    if (!h || ch >= h->nch)
        return fail(PSK_SOFT_ERR_INVALID_ARG, "psk_soft_fire_listener: bad channel");
    ctl_touch(h);
    switch (which) {
    case 0: h->ctl[ch].samplesPerBaudChanged(); break;
    case 1: h->ctl[ch].constelationSizeChanged(); break;
    case 2: h->ctl[ch].phaseAvgChanged(); break;
    default: return fail(PSK_SOFT_ERR_INVALID_ARG, "psk_soft_fire_listener: which must be 0..2");
    }
    return PSK_SOFT_OK;
}

uint64_t psk_soft_output_capacity(const psk_soft_handle_t *h, uint32_t ch, uint64_t n_complex)
{
    if (!h || ch >= h->nch)
        return 0;
    ctl_sync(h);
    uint64_t S = h->ctl[ch].props.samplesPerBaud ? h->ctl[ch].props.samplesPerBaud : 1;
    return (n_complex + S - 1) / S + 1;
}

// The call behind the public entry (psk_soft_process_device, below).  A call that would emit more than 2^20 symbols in one channel, or run LinearFit::count past 2^20 in the
// middle (the reference then rebuilds the fit's sums at that symbol, cpp/psk_soft.cpp:51-52, and its energy sums after it,
// :582-583), is cut at those boundaries inside the library: the pieces are planned as continuations of ONE serviceFunction() call
// (no prologue between them) and run on the wave-scan / time-tiled kernels like any other call -- round 2 handed such calls to the
// reference-order kernel, 4.7 us per symbol on one lane.  Everything else goes straight through.
static psk_soft_status process_device_call(psk_soft_handle_t *h, uint32_t ch0, uint32_t nch, const psk_soft_packet_t *pkts,
                                           psk_soft_output_t *outs, void *stream_v)
{
    // (the ordinary call is planned as it is; the plan pass itself says when a channel's call is too long for one piece --
    // nothing is committed or enqueued then)
    Verdict verdict;
    {
        const psk_soft_status st = process_round(h, ch0, nch, pkts, outs, stream_v, Pieces{}, &verdict);
        if (st != PSK_SOFT_OK || verdict.what == Verdict::done)
            return st;
    }
    // (a mixed batch cut in time, see Verdict: every channel's call in `split` pieces of whole blocks; the side streams of
    // the rounds are joined once, behind the last)
    const uint64_t split = verdict.what == Verdict::mixed ? (uint64_t)verdict.pieces : 0;
    std::vector<uint64_t> piece_cap(split ? nch : 0, ~0ull);  // symbols a piece of the channel's call may emit

    // ---- pieces ----
    ctl_sync(h);
    std::vector<psk_soft_packet_t> pk(pkts, pkts + nch);
    std::vector<psk_soft_output_t> ou(outs, outs + nch), total(outs, outs + nch);
    std::vector<uint64_t> left(nch);   // floats of the packet not yet handed over
    std::vector<uint8_t> cont(nch, 0);
    std::vector<uint32_t> mode_of(nch, psk::PLAN_SKIP);  // (statistics: the kernel of each channel's last piece)
    for (uint32_t i = 0; i < nch; i++) left[i] = pkts[i].present ? pkts[i].n_floats : 0;
    for (int round = 0;; round++) {
        bool more = false;
        for (uint32_t i = 0; i < nch; i++) {
            psk_soft_packet_t &q = pk[i];
            if (round > 0) {
                q.present = left[i] ? 1 : 0;  // (a channel whose packet is used up sits the later rounds out)
                q.sriChanged = 0;
                q.inputQueueFlushed = 0;
            }
            cont[i] = round > 0 ? (split ? 5 : 1) : 0;  // (bit 2: the bounds of the call so far carry over, PLAN_CARRY_DRIFT)
            if (!q.present || q.sri_mode != 1) {
                left[i] = 0;
                continue;
            }
            const psk::ChanCtl &c = h->ctl[ch0 + i];
            const uint64_t S = c.props.samplesPerBaud ? c.props.samplesPerBaud : 1, A = c.props.numAvg;
            // the first round runs the call's prologue, which (quirk Q2) resets LinearFit::count in practically every call: plan on a
            // copy to learn what this piece would emit, and shorten it to an even number of symbols within the limit (the output
            // rows of the next piece must stay 4-byte aligned: bits and sampleIndex are 2 bytes a symbol)
            uint64_t n_fl = left[i];
            for (int attempt = 0; attempt < 4; attempt++) {
                psk::ChanCtl probe = c;
                psk::ChanPlan pl;
                psk_soft_packet_t qq = q;
                qq.n_floats = n_fl;
                psk_soft_output_t oo = ou[i];
                oo.cap_symbols = ~0ull;
                if (psk::plan_call(probe, h->lim, qq, oo, pl, (cont[i] & 1u) != 0) != PSK_SOFT_OK)
                    break;  // (the real pass reports it)
                uint64_t lim_sym = psk::kResyncCount - pl.lf_count0 < psk::kResyncCount ? psk::kResyncCount - pl.lf_count0 : psk::kResyncCount;
                if (split) {
                    if (round == 0 && attempt == 0)  // (the whole call's symbols: pieces of whole blocks, `split` of them)
                        piece_cap[i] = ((oo.n_symbols + split - 1) / split + 127ull) & ~127ull;
                    lim_sym = piece_cap[i] < lim_sym ? piece_cap[i] : lim_sym;
                }
                const bool last = n_fl == left[i];
                if (oo.n_symbols <= lim_sym && (last || (oo.n_symbols & 1ull) == 0))
                    break;
                // too many (or an odd number of) symbols: give the piece fewer samples
                uint64_t want = oo.n_symbols > lim_sym ? lim_sym : oo.n_symbols - 1;
                want &= ~1ull;
                const uint64_t excess = oo.n_symbols - want;
                const uint64_t cut = 2ull * S * excess;
                n_fl = n_fl > cut ? n_fl - cut : 2ull * S * (A + 2);
                (void)A;
            }
            // (a piece that is not the last holds whole complex samples: an odd element at the end of the packet goes with the last
            // piece, which ignores it -- in an earlier one it would start the next piece one element late, misaligned)
            if (n_fl < left[i])
                n_fl &= ~1ull;
            q.n_floats = n_fl;
            left[i] -= n_fl < left[i] ? n_fl : left[i];
            if (left[i])
                cont[i] |= 2u;
            more = more || left[i] != 0;
        }
        const psk_soft_status st = process_round(h, ch0, nch, pk.data(), ou.data(), stream_v, Pieces{cont.data(), split != 0}, &verdict);
        if (st != PSK_SOFT_OK) {
            if (round > 0)
                h->poisoned = true;  // (pieces of the call have run: the channels are in the middle of it)
            return st;
        }
        ctl_sync(h);
        for (uint32_t i = 0; i < nch; i++) {
            const psk_soft_output_t &o = ou[i];
            psk_soft_output_t &t = total[i];
            if (round == 0) {
                t = o;
                t.soft = outs[i].soft, t.bits = outs[i].bits, t.phase = outs[i].phase, t.sampleIndex = outs[i].sampleIndex;
                t.cap_symbols = outs[i].cap_symbols;
            } else if (pk[i].present) {
                t.n_symbols += o.n_symbols;
                t.n_bits += o.n_bits;
                t.n_sampleIndex += o.n_sampleIndex;
                t.n_warn += o.n_warn;
            }
            // the next piece reads and writes behind this one
            if (pk[i].present) {
                mode_of[i] = h->last_mode[ch0 + i];
                pk[i].data = pk[i].data ? reinterpret_cast<const float *>(reinterpret_cast<const char *>(pk[i].data) +
                                                                          elem_bytes(pk[i]) * pk[i].n_floats)
                                        : nullptr;
                pk[i].n_floats = left[i];
                if (ou[i].soft) ou[i].soft += 2 * o.n_symbols;
                if (ou[i].bits) ou[i].bits += o.n_bits;
                if (ou[i].phase) ou[i].phase += o.n_symbols;
                if (ou[i].sampleIndex) ou[i].sampleIndex += o.n_sampleIndex;
                ou[i].cap_symbols = ou[i].cap_symbols > o.n_symbols ? ou[i].cap_symbols - o.n_symbols : 0;
            }
        }
        if (!more)
            break;
    }
    ctl_sync(h);
    for (uint32_t i = 0; i < nch; i++) {
        outs[i] = total[i];
        h->last_mode[ch0 + i] = mode_of[i];
    }
    if (split && !h->dry && !h->opt_deferred) {  // (the call ends like any other: the caller's stream behind all of it)
        PSK_HIP(hipSetDevice(h->device));
        PSK_HIP(deferred_join(h, stream_v ? (hipStream_t)stream_v : h->stream));
    }
    return PSK_SOFT_OK;
}

// PSK_SOFT_OPT_QUALITY: the reduction pass behind a call (psk_quality.hip) -- fold + join on the caller's stream over the call's
// WHOLE rows (the pointers and total counts of outs[]: the pass does not care how the call was scheduled), one record per channel
// of the call.  The descriptors go up from pinned memory of a slot of their own, reused behind its event.
static psk_soft_status quality_pass(psk_soft_handle_t *h, uint32_t ch0, uint32_t nch, const psk_soft_output_t *outs, void *stream_v)
{
    const psk_soft_handle::QualitySnap *snap = h->q_snap.data();
    if (h->dry) {
        for (uint32_t i = 0; i < nch; i++) {
            psk_soft_quality_t r = {};
            r.n_symbols = outs[i].n_symbols;
            r.constelationSize = snap[i].M, r.samplesPerBaud = snap[i].S, r.differentialDecoding = snap[i].diff;
            r.flags = PSK_SOFT_Q_PLANNED;
            h->quality.dry[ch0 + i] = r;
        }
        return PSK_SOFT_OK;
    }
    PSK_HIP(hipSetDevice(h->device));
    hipStream_t stream = stream_v ? (hipStream_t)stream_v : h->stream;
    // (a deferred call's classes end on the side streams: the rows must be complete)
    PSK_HIP(deferred_join(h, stream));
    auto &q = h->qpass.next();
    PSK_TRY(h->qpass.claim(q, h->nch));
    PieceCount segs;  // (the pieces of this pass: segments of kQualitySegSymbols symbols)
    for (uint32_t i = 0; i < nch; i++) {
        const psk_soft_output_t &o = outs[i];
        psk::QualityDesc &d = q.h_desc[i];
        d = psk::QualityDesc{};
        d.channel = ch0 + i;
        d.M = snap[i].M, d.S = snap[i].S, d.diff = snap[i].diff;
        if (!o.n_symbols)
            continue;  // (its zero record)
        d.n_symbols = o.n_symbols;
        d.n_sidx = o.n_sampleIndex;
        uint32_t f = 0;
        if (o.soft)
            f |= PSK_SOFT_Q_SOFT | (d.M == 2 || d.M == 4 || d.M == 8 ? PSK_SOFT_Q_LOCK : 0);
        if (o.phase)
            f |= PSK_SOFT_Q_PHASE;
        if (o.sampleIndex && o.n_sampleIndex)
            f |= PSK_SOFT_Q_INDEX;
        d.flags = (uint8_t)f;
        d.soft = (f & PSK_SOFT_Q_SOFT) ? o.soft : nullptr;
        d.phase = (f & PSK_SOFT_Q_PHASE) ? o.phase : nullptr;
        d.sidx = (f & PSK_SOFT_Q_INDEX) ? o.sampleIndex : nullptr;
        if ((f & (PSK_SOFT_Q_SOFT | PSK_SOFT_Q_INDEX)) &&
            !segs.add((o.n_symbols + psk::kQualitySegSymbols - 1u) / psk::kQualitySegSymbols, &d.seg0, &d.n_seg))
            return fail(PSK_SOFT_ERR_LIMIT, "psk_soft_process: too many symbols in one call for the quality pass");
    }
    // (PSK_SOFT_TRACE_LAUNCHES, trace_launch: tiles = segments; `slot` is the call's last plan slot)
    auto mark = [&](const char *what) { return trace_launch(h, what, 0, 0, ch0, nch, segs.total, 0, 0, (h->slot + kPlanSlots - 1) % kPlanSlots, stream); };
    return h->qpass.run(q, nch, {ch0, nch}, segs.total, stream, [&]() -> psk_soft_status {
        PSK_HIP(mark("quality_fold"));
        PSK_HIP(psk::launch_quality_fold(q.d_desc, nch, segs.max_piece, q.d_part, stream));
        PSK_HIP(mark("quality_join"));
        PSK_HIP(psk::launch_quality_join(q.d_desc, nch, q.d_part, h->quality.d, stream));
        return PSK_SOFT_OK;
    });
}

// The public entry: the call, and with PSK_SOFT_OPT_QUALITY the reduction pass behind it.
psk_soft_status psk_soft_process_device(psk_soft_handle_t *h, uint32_t ch0, uint32_t nch,
                                        const psk_soft_packet_t *pkts, psk_soft_output_t *outs, void *stream_v)
{
    if (!h || !pkts || !outs || !nch || (uint64_t)ch0 + nch > h->nch)
        return fail(PSK_SOFT_ERR_INVALID_ARG, "psk_soft_process: bad arguments");
    if (!h->opt_quality)
        return process_device_call(h, ch0, nch, pkts, outs, stream_v);
    // (the properties the call runs with: it snapshots them at its top, reference cpp/psk_soft.cpp:374-378)
    h->q_snap.resize(nch);
    for (uint32_t i = 0; i < nch; i++) {
        const psk_soft_props_t &p = ctl_of(h, ch0 + i).props;
        h->q_snap[i] = {p.constelationSize, p.samplesPerBaud, (uint8_t)(p.differentialDecoding != 0)};
    }
    const psk_soft_status st = process_device_call(h, ch0, nch, pkts, outs, stream_v);
    if (st != PSK_SOFT_OK)
        return st;
    return quality_pass(h, ch0, nch, outs, stream_v);
}

// The refusals of a strided argument, for the entries that take one: a stride of 0; for a packet of a known format (what an entry does
// with an unknown one is its own business) an extent that does not fit 64 bits, and -- `read`: the call reads the packet's samples --
// data that do not start on a whole sample.  ch: the channel, s: its stride.
struct StridedEntry {
    const char *name, *misaligned;  // the entry in the messages about strides; its whole message about alignment
};
static const StridedEntry kProcessEntry = {"psk_soft_process_device_strided", "psk_soft_process: packet data must be 8-byte aligned (CS16: 4) (CS8: 2) (CF16: 4), soft 8, bits 4, phase 4, sampleIndex 4"};
static const StridedEntry kAcquireEntry = {"psk_soft_acquire_device", "psk_soft_acquire_device: packet data must be 8-byte aligned (CS16: 4) (CS8: 2) (CF16: 4)"};
static psk_soft_status strided_refusal(const StridedEntry &e, uint32_t ch, const psk_soft_packet_t &k, uint64_t s, bool read)
{
    char buf[160];
    if (!s) {
        std::snprintf(buf, sizeof buf, "%s: channel %u: a sample stride of 0", e.name, ch);
        return fail(PSK_SOFT_ERR_INVALID_ARG, buf);
    }
    if (!psk::pkt_format_known(k.format))
        return PSK_SOFT_OK;
    const uint64_t sb = 2u * elem_bytes(k);
    uint64_t pitch = 0, extent = 0;
    if (__builtin_mul_overflow(s, sb, &pitch) || __builtin_mul_overflow(pitch, k.n_floats / 2u, &extent)) {
        std::snprintf(buf, sizeof buf, "%s: channel %u: stride x sample size x samples does not fit 64 bits", e.name, ch);
        return fail(PSK_SOFT_ERR_INVALID_ARG, buf);
    }
    if (read && reinterpret_cast<uintptr_t>(k.data) % sb)
        return fail(PSK_SOFT_ERR_INVALID_ARG, e.misaligned);
    return PSK_SOFT_OK;
}

// tuned packets: the two phasor tables in device memory (once per handle)
static psk_soft_status ensure_tune_tab(psk_soft_handle *h)
{
    if (h->d_tune_tab)
        return PSK_SOFT_OK;
    PSK_HIP(h->d_tune_tab.alloc(psk::kTuneTableFloats));
    PSK_HIP(hipMemcpy(h->d_tune_tab, psk::tune_tables(), sizeof(float) * psk::kTuneTableFloats, hipMemcpyHostToDevice));
    return PSK_SOFT_OK;
}

// ---- the front stages of a call: gathers, tune, filter, resample (psk_soft_process_device_filtered, psk_soft_acquire_device) ----
// A call is classified once (front_classify: which kernel reads each packet, what the ordinary call sees in its place, the
// refusals) and the plan is then read by one function per step, in the order a call goes through them: front_layout,
// front_describe, front_launch, front_release, front_commit.  DESIGN.md 2.11.
struct FrontCall {
    psk_soft_handle *h;
    uint32_t ch0, nch;
    const psk_soft_packet_t *pkts;
    const uint64_t *sample_stride;  // NULL: every packet contiguous
    const psk_soft_tune_t *tune;    // NULL: none tuned
    const psk_soft_fir_t *fir;
    const psk_soft_resample_t *resample;
    hipStream_t stream;
    uint64_t stride(uint32_t i) const { return sample_stride ? sample_stride[i] : 1u; }
    // packet i has a tune: its {phase, step} is not {0, 0}
    bool has_tune(uint32_t i) const { return tune && (tune[i].phase | tune[i].step) != 0; }
};

// One packet of the call.  At most one of tune / fir reads it, the resample kernel reads it or the filter's row of it; all false:
// the ordinary call gets the packet as it is (or its gathered row).
struct FrontPkt {
    bool gathered = false;  // strided and read: a column of a frame group, or a strided single
    bool tune = false;      // the tune kernel reads it (tuned, neither filtered nor resampled)
    bool fir = false;       // the filter kernel reads it
    bool resample = false;  // the resample kernel reads it, or the row the filter has made of it
    bool has_tune = false;  // whichever of the three reads it first rotates it
    bool data = false;      // it has data -- or the handle is control-plane-only, which never looks
    uint64_t n_in = 0, n_fir = 0, n_out = 0;  // samples: of the packet, behind the filter, of what the ordinary call sees
    // front_layout: offsets into the scratch of its own-format row (has_own), the filter's float2 row, the last float2 row
    bool has_own = false, in_group = false;
    size_t own_off = 0, fir_off = 0, f2_off = 0;
    // front_describe: the rows themselves (nullptr: none)
    const void *own_row = nullptr;
    float *f2_row = nullptr;  // the row the ordinary call reads: the tune kernel's, the resampler's, else the filter's
};

struct FrontPlan {
    std::vector<FrontPkt> pkt;
    uint32_t n_gather = 0, n_tune = 0, n_fir = 0, n_rs = 0;
    bool unknown = false;  // a strided packet of an unknown format: the whole call is the ordinary call's to refuse
    bool rotates = false;  // a filtered or resampled packet has a tune: those kernels need the tables
    // a strided single is read where it lies by the caller's own kernel (psk_soft_acquire_device): no row, no gather
    bool singles_in_place = false;
    // frame groups: maximal runs of gathered packets of one format and stride whose data lie one sample apart
    struct Run {
        uint32_t first, g, bytes;
    };
    std::vector<Run> runs;
    size_t need = 0;  // bytes of scratch
    // descriptors, per sample size (2, 4, 8 bytes: one launch of each gather kernel per size):
    // [groups | their columns | singles | tune | resample | fir]
    uint32_t n_groups[3] = {}, n_cols[3] = {}, n_singles[3] = {};
    size_t off_cols = 0, off_singles = 0, off_tune = 0, off_rs = 0, off_fir = 0, desc_bytes = 0;
    uint64_t n_tiles[3] = {}, max_n_single[3] = {}, max_n_tune = 0, max_n_rs = 0, max_fir_pieces = 0;
    StreamScratch *sc = nullptr;
    GatherDescSlot *ds = nullptr;
    bool owed = false;  // the descriptors are on the stream: front_release is owed

    bool nothing() const { return !n_gather && !n_tune && !n_fir && !n_rs; }
    bool direct(uint32_t i) const { return singles_in_place || pkt[i].tune || pkt[i].fir || pkt[i].resample; }
    static int size_idx(uint32_t bytes) { return bytes == 2 ? 0 : bytes == 4 ? 1 : 2; }
};

// Classifies the packets of a process call, one pass, no HIP call.  The refusals of the entry come out of it, before anything is
// planned: per packet the filter's, the resampler's, then a stride of 0, an extent that does not fit 64 bits, data that do not
// start on a whole sample.  (A packet of an unknown format is left to the ordinary call, which refuses it.)
static psk_soft_status front_classify(const FrontCall &c, FrontPlan &plan)
{
    const psk_soft_handle *h = c.h;
    plan.pkt.assign(c.nch, FrontPkt{});
    for (uint32_t i = 0; i < c.nch; i++) {
        const psk_soft_packet_t &k = c.pkts[i];
        FrontPkt &p = plan.pkt[i];
        if (!k.present)
            continue;
        p.data = k.data || h->dry;
        p.has_tune = c.has_tune(i);
        p.n_in = p.n_fir = p.n_out = k.n_floats / 2u;
        // (a packet a front kernel can read: complex data, at least one sample, of a format the library knows)
        const bool known = psk::pkt_format_known(k.format);
        const bool reads = k.sri_mode == 1 && k.n_floats >= 2 && known && p.data;
        char buf[160];
        if (c.fir && c.fir[i].filter != 0) {
            const psk_soft_fir_t &f = c.fir[i];
            const char *what = f.filter > psk::kFirSlots || !h->fir_ntaps[f.filter - 1u] ? "a filter slot that is not defined"
                               : !f.decim || f.decim > psk::kFirMaxDecim                 ? "a decimation outside 1 .. 16"
                               : f.pos >= f.decim                                        ? "a position not below the decimation"
                               : (f.flags & ~(uint32_t)PSK_SOFT_FIR_RESTART)             ? "unknown flag bits"
                               : p.n_in >= psk::kFirMaxN                                 ? "2^30 samples or more"
                                                                                         : nullptr;
            if (what) {
                std::snprintf(buf, sizeof buf, "psk_soft_process_device_filtered: channel %u: %s", c.ch0 + i, what);
                return fail(PSK_SOFT_ERR_INVALID_ARG, buf);
            }
            p.n_fir = p.n_out = psk::fir_count(f.pos, f.decim, p.n_in);
            p.fir = reads;
        }
        if (c.resample && c.resample[i].step != 0) {
            const psk_soft_resample_t &r = c.resample[i];
            const char *what = r.step < psk::kResampleStepMin || r.step > psk::kResampleStepMax ? "a step outside [2^31, 2^33]"
                               : r.pos > psk::kResamplePosMax                                  ? "a position above 2^33"
                               : p.n_in >= psk::kResampleMaxN                                  ? "2^30 samples or more"
                               : r.pad                                                         ? "a non-zero pad"
                               : (r.flags & ~(uint32_t)PSK_SOFT_RS_RESTART)                    ? "unknown flag bits"
                                                                                               : nullptr;
            if (what) {
                std::snprintf(buf, sizeof buf, "psk_soft_process_device_resampled: channel %u: %s", c.ch0 + i, what);
                return fail(PSK_SOFT_ERR_INVALID_ARG, buf);
            }
            // (a filter without outputs leaves the resampler nothing: its packet is the filter's alone)
            if (reads && p.n_fir != 0) {
                p.resample = true;
                p.n_out = psk::resample_count(r.pos, r.step, p.n_fir);
            }
        }
        // (a packet both tuned and filtered or resampled is tuned inside the first of those kernels that reads it)
        p.tune = p.has_tune && reads && !p.fir && !p.resample;
        const uint64_t s = c.stride(i);
        if (s == 1) {  // (contiguous: the ordinary call's business, but for the packets a front kernel reads)
            if ((p.tune || p.fir || p.resample) && reinterpret_cast<uintptr_t>(k.data) % (2u * elem_bytes(k)))
                return fail(PSK_SOFT_ERR_INVALID_ARG, kProcessEntry.misaligned);
        } else {
            p.gathered = k.sri_mode == 1 && k.n_floats >= 2 && p.data;
            PSK_TRY(strided_refusal(kProcessEntry, c.ch0 + i, k, s, p.gathered));
            if (!known) {
                plan.unknown = true;
                continue;
            }
        }
        plan.n_gather += p.gathered, plan.n_tune += p.tune, plan.n_fir += p.fir, plan.n_rs += p.resample;
        plan.rotates |= p.has_tune && (p.fir || p.resample);
    }
    return PSK_SOFT_OK;
}

// The copy of the packet array the ordinary call runs on.  It sees a filtered or resampled packet as CF32 with the samples and the
// sample period behind those stages; with `rows` (a control-plane-only handle has none: lengths, formats and sample periods are
// all it looks at) a packet a front kernel has written points at its last float2 row, a tuned one as CF32, and any other
// gathered packet at its own-format row.
static void front_packets(const FrontCall &c, const FrontPlan &plan, bool rows, std::vector<psk_soft_packet_t> &pk)
{
    pk.assign(c.pkts, c.pkts + c.nch);
    for (uint32_t i = 0; i < c.nch; i++) {
        const FrontPkt &p = plan.pkt[i];
        psk_soft_packet_t &k = pk[i];
        if (p.fir)
            k.sri_xdelta = k.sri_xdelta * (double)c.fir[i].decim;
        if (p.resample)
            k.sri_xdelta = k.sri_xdelta * ((double)c.resample[i].step * 0x1p-32);
        if (p.fir || p.resample || (rows && p.tune)) {
            k.n_floats = 2u * p.n_out;
            k.format = PSK_SOFT_FORMAT_CF32;
        }
        if (rows && p.f2_row)
            k.data = p.f2_row;
        else if (rows && p.own_row)
            k.data = reinterpret_cast<const float *>(p.own_row);
    }
}

// 1. Layout: the frame groups among the gathered packets, the rows of the scratch and the descriptor block.  A column of a run of at
// least kGatherMinGroup goes through the tile kernel into its own-format row.  A column of a shorter run goes through the plain
// strided gather, unless a front kernel reads it where it lies (FrontPlan::direct: it gets no own-format row).  Every row starts
// on a 128-byte boundary; a float2 row holds its kernel's outputs (a tuned packet's samples), one sample's room at the least.
static void front_layout(const FrontCall &c, FrontPlan &plan)
{
    auto row_bytes = [](uint64_t n) { return align_up(sizeof(float2) * (size_t)(n ? n : 1u), 128); };
    auto f2_rows = [&](FrontPkt &p) {
        if (p.fir) {
            p.fir_off = plan.need;
            plan.need += row_bytes(p.n_fir);
        }
        if (p.tune || p.resample) {
            p.f2_off = plan.need;
            plan.need += row_bytes(p.n_out);
        }
    };
    for (uint32_t i = 0; i < c.nch;) {
        if (!plan.pkt[i].gathered) {
            f2_rows(plan.pkt[i]);
            i++;
            continue;
        }
        const uint32_t sb = 2u * (uint32_t)elem_bytes(c.pkts[i]);
        uint32_t j = i + 1;
        while (j < c.nch && plan.pkt[j].gathered && c.pkts[j].format == c.pkts[i].format && c.sample_stride[j] == c.sample_stride[i] &&
               reinterpret_cast<const char *>(c.pkts[j].data) == reinterpret_cast<const char *>(c.pkts[j - 1].data) + sb)
            j++;
        plan.runs.push_back({i, j - i, sb});
        const bool group = j - i >= psk::kGatherMinGroup;
        const int b = FrontPlan::size_idx(sb);
        if (group)
            plan.n_groups[b]++, plan.n_cols[b] += j - i;
        for (uint32_t k = i; k < j; k++) {
            FrontPkt &p = plan.pkt[k];
            p.in_group = group;
            if (group || !plan.direct(k)) {
                p.own_off = plan.need;
                p.has_own = true;
                plan.need += align_up((size_t)sb * p.n_in, 128);
                plan.n_singles[b] += !group;
            }
            f2_rows(p);
        }
        i = j;
    }
    const uint32_t tot_groups = plan.n_groups[0] + plan.n_groups[1] + plan.n_groups[2];
    const uint32_t tot_cols = plan.n_cols[0] + plan.n_cols[1] + plan.n_cols[2];
    const uint32_t tot_singles = plan.n_singles[0] + plan.n_singles[1] + plan.n_singles[2];
    plan.off_cols = sizeof(psk::GatherGroup) * tot_groups;
    plan.off_singles = plan.off_cols + sizeof(psk::GatherChan) * tot_cols;
    plan.off_tune = plan.off_singles + sizeof(psk::GatherSingle) * tot_singles;
    plan.off_rs = plan.off_tune + sizeof(psk::TuneDesc) * plan.n_tune;
    plan.off_fir = plan.off_rs + sizeof(psk::ResampleDesc) * plan.n_rs;
    plan.desc_bytes = plan.off_fir + sizeof(psk::FirDesc) * plan.n_fir;
}

// 2. Describe: claims the stream's scratch (its own buffer, else the one used longest ago, behind the event of its last call) and a
// descriptor slot, and fills the pinned descriptors.  The tune, filter and resample kernels read a column of a frame group from
// the row the tile kernel writes, any other packet where the caller has it, at its stride; a packet both filtered and resampled
// is resampled from its filter row.
static psk_soft_status front_describe(const FrontCall &c, FrontPlan &plan)
{
    psk_soft_handle *h = c.h;
    // PSK_SOFT_OPT_DEFERRED_JOIN: a class of an earlier call may still be reading its rows on a side stream -- joined first
    PSK_HIP(deferred_join(h, c.stream));
    PSK_TRY(claim_scratch(h->gat, &h->gat_calls, c.stream, plan.need, nullptr, &plan.sc));
    if (plan.n_tune || plan.rotates)
        PSK_TRY(ensure_tune_tab(h));
    if (plan.n_rs)
        PSK_TRY(h->rs_hist.ensure(h->nch));
    if (plan.n_fir)
        PSK_TRY(h->fir_hist.ensure(h->nch));
    GatherDescSlot &ds = h->gdesc[h->gdesc_turn];
    h->gdesc_turn = (h->gdesc_turn + 1) % kGatherDescSlots;
    PSK_TRY(ds.claim(plan.desc_bytes));
    plan.ds = &ds;
    char *const buf = plan.sc->buf;
    psk::GatherGroup *const hg = reinterpret_cast<psk::GatherGroup *>(ds.h_buf.get());
    psk::GatherChan *const hc = reinterpret_cast<psk::GatherChan *>(ds.h_buf + plan.off_cols);
    psk::GatherSingle *const hs = reinterpret_cast<psk::GatherSingle *>(ds.h_buf + plan.off_singles);
    psk::TuneDesc *ht = reinterpret_cast<psk::TuneDesc *>(ds.h_buf + plan.off_tune);
    psk::ResampleDesc *hr = reinterpret_cast<psk::ResampleDesc *>(ds.h_buf + plan.off_rs);
    psk::FirDesc *hf = reinterpret_cast<psk::FirDesc *>(ds.h_buf + plan.off_fir);
    // (the launch of a sample size gets the groups, columns and singles of that size: they lie together, sizes in ascending order)
    uint32_t g_at[3] = {0, plan.n_groups[0], plan.n_groups[0] + plan.n_groups[1]};
    uint32_t c_at[3] = {0, plan.n_cols[0], plan.n_cols[0] + plan.n_cols[1]};
    uint32_t s_at[3] = {0, plan.n_singles[0], plan.n_singles[0] + plan.n_singles[1]};
    const uint32_t c_lo[3] = {c_at[0], c_at[1], c_at[2]};
    for (const FrontPlan::Run &r : plan.runs) {
        const int b = FrontPlan::size_idx(r.bytes);
        psk::GatherGroup *g = nullptr;
        if (r.g >= psk::kGatherMinGroup) {
            g = &hg[g_at[b]++];
            *g = psk::GatherGroup{};
            g->src = c.pkts[r.first].data;
            g->stride = c.sample_stride[r.first];
            g->first = c_at[b] - c_lo[b];
            g->g = r.g;
            g->tiles_c = (r.g + psk::kGatherTile - 1u) / psk::kGatherTile;
        }
        for (uint32_t k = r.first; k < r.first + r.g; k++) {
            FrontPkt &p = plan.pkt[k];
            if (!p.has_own)
                continue;
            p.own_row = buf + p.own_off;
            if (g) {
                hc[c_at[b]++] = psk::GatherChan{buf + p.own_off, p.n_in};
                g->n_max = p.n_in > g->n_max ? p.n_in : g->n_max;
            } else {
                hs[s_at[b]++] = psk::GatherSingle{c.pkts[k].data, buf + p.own_off, c.sample_stride[k], p.n_in};
                plan.max_n_single[b] = p.n_in > plan.max_n_single[b] ? p.n_in : plan.max_n_single[b];
            }
        }
        if (g) {
            g->tile0 = plan.n_tiles[b];
            plan.n_tiles[b] += (uint64_t)g->tiles_c * ((g->n_max + psk::kGatherTile - 1u) / psk::kGatherTile);
        }
    }
    for (uint32_t i = 0; i < c.nch; i++) {
        FrontPkt &p = plan.pkt[i];
        if (!p.tune && !p.fir && !p.resample)
            continue;
        // the packet as its first kernel reads it
        psk::FrontIo io = {};
        io.src = p.in_group ? (const void *)(buf + p.own_off) : (const void *)c.pkts[i].data;
        io.stride = p.in_group ? 1u : c.stride(i);
        io.n = p.n_in;
        io.format = c.pkts[i].format;
        if (p.has_tune)
            io.phase = c.tune[i].phase, io.step = c.tune[i].step, io.flags = p.tune ? 0u : psk::kFrontTuned;
        if (p.tune) {
            io.dst = p.f2_row = reinterpret_cast<float *>(buf + p.f2_off);
            *ht++ = io;
            plan.max_n_tune = io.n > plan.max_n_tune ? io.n : plan.max_n_tune;
            continue;
        }
        if (p.fir) {
            const psk_soft_fir_t &f = c.fir[i];
            psk::FirDesc &d = *hf++;
            d = psk::FirDesc{};
            d.io = io;
            d.io.dst = p.f2_row = reinterpret_cast<float *>(buf + p.fir_off);
            d.io.flags |= (f.flags & PSK_SOFT_FIR_RESTART) ? psk::kFrontRestart : 0u;
            d.decim = f.decim, d.pos = f.pos, d.n_taps = h->fir_ntaps[f.filter - 1u], d.n_out = p.n_fir;
            d.taps = h->d_fir_taps + (size_t)psk::kFirMaxTaps * (f.filter - 1u);
            d.hist_in = h->fir_hist.in(c.ch0 + i), d.hist_out = h->fir_hist.out(c.ch0 + i);
            const uint32_t piece = psk::fir_piece(d.decim);
            const uint64_t pieces = (d.n_out + piece - 1u) / piece;
            plan.max_fir_pieces = pieces > plan.max_fir_pieces ? pieces : plan.max_fir_pieces;
            if (!p.resample)
                continue;
            // (the resampler reads the filter's outputs, which are tuned already)
            io = psk::FrontIo{};
            io.src = d.io.dst, io.stride = 1u, io.n = p.n_fir, io.format = PSK_SOFT_FORMAT_CF32;
        }
        const psk_soft_resample_t &r = c.resample[i];
        psk::ResampleDesc &d = *hr++;
        d = psk::ResampleDesc{};
        d.io = io;
        d.io.dst = p.f2_row = reinterpret_cast<float *>(buf + p.f2_off);
        d.io.flags |= (r.flags & PSK_SOFT_RS_RESTART) ? psk::kFrontRestart : 0u;
        d.pos = r.pos, d.rstep = r.step, d.n_out = p.n_out;
        d.hist_in = h->rs_hist.in(c.ch0 + i), d.hist_out = h->rs_hist.out(c.ch0 + i);
        plan.max_n_rs = d.n_out > plan.max_n_rs ? d.n_out : plan.max_n_rs;
    }
    return PSK_SOFT_OK;
}

// 3. Launch: the descriptors in one copy, then the gathers per sample size, the tune kernel, the filter kernel and the resample
// kernel, all on the call's stream; the histories' events behind their kernels.
static psk_soft_status front_launch(const FrontCall &c, FrontPlan &plan)
{
    psk_soft_handle *h = c.h;
    GatherDescSlot &ds = *plan.ds;
    PSK_HIP(hipMemcpyAsync(ds.d_buf, ds.h_buf, plan.desc_bytes, hipMemcpyHostToDevice, c.stream));
    plan.owed = true;  // (from here on the slot waits for its event, which front_release records whatever happens)
    // (PSK_SOFT_TRACE_LAUNCHES, trace_launch: S = bytes of a complex sample, cnt = groups / singles / packets covered)
    auto mark = [&](const char *what, int bytes, uint32_t cnt, uint64_t tiles) {
        return trace_launch(h, what, bytes, 0, c.ch0, cnt, tiles, 0, 0, h->slot, c.stream);
    };
    const psk::GatherGroup *dg = reinterpret_cast<const psk::GatherGroup *>(ds.d_buf.get());
    const psk::GatherChan *dc = reinterpret_cast<const psk::GatherChan *>(ds.d_buf + plan.off_cols);
    const psk::GatherSingle *dsg = reinterpret_cast<const psk::GatherSingle *>(ds.d_buf + plan.off_singles);
    for (int b = 0; b < 3; b++) {
        const int bytes = 2 << b;
        if (plan.n_groups[b]) {
            PSK_HIP(mark("gather_tiles", bytes, plan.n_groups[b], plan.n_tiles[b]));
            PSK_HIP(psk::launch_gather_tiles(bytes, dg, plan.n_groups[b], dc, plan.n_tiles[b], c.stream));
        }
        if (plan.n_singles[b]) {
            PSK_HIP(mark("gather_singles", bytes, plan.n_singles[b], 0));
            PSK_HIP(psk::launch_gather_singles(bytes, dsg, plan.n_singles[b], plan.max_n_single[b], c.stream));
        }
        dg += plan.n_groups[b], dc += plan.n_cols[b], dsg += plan.n_singles[b];
    }
    if (plan.n_tune) {
        PSK_HIP(mark("tune", 8, plan.n_tune, 0));
        PSK_HIP(psk::launch_tune(reinterpret_cast<const psk::TuneDesc *>(ds.d_buf + plan.off_tune), plan.n_tune, plan.max_n_tune, h->d_tune_tab, c.stream));
    }
    if (plan.n_fir) {
        PSK_HIP(mark("fir", 8, plan.n_fir, 0));
        PSK_HIP(psk::launch_fir(reinterpret_cast<const psk::FirDesc *>(ds.d_buf + plan.off_fir), plan.n_fir, plan.max_fir_pieces, h->d_tune_tab, c.stream));
        PSK_TRY(h->fir_hist.record(c.stream));
    }
    if (plan.n_rs) {
        PSK_HIP(mark("resample", 8, plan.n_rs, 0));
        PSK_HIP(psk::launch_resample(reinterpret_cast<const psk::ResampleDesc *>(ds.d_buf + plan.off_rs), plan.n_rs, plan.max_n_rs, h->d_tune_tab, c.stream));
        PSK_TRY(h->rs_hist.record(c.stream));
    }
    return PSK_SOFT_OK;
}

// Steps 1 to 3.  A call with nothing to launch returns before it touches a stream, plan.owed == false.
static psk_soft_status front_enqueue(const FrontCall &c, FrontPlan &plan)
{
    front_layout(c, plan);
    if (!plan.desc_bytes)
        return PSK_SOFT_OK;
    PSK_TRY(front_describe(c, plan));
    return front_launch(c, plan);
}

// 4. Release: the rows and the descriptors are free again behind everything the call has put on the stream (without the deferred
// join the side streams of a process call are joined into it by now; with it, the next call that gathers joins them first, in
// front_describe).  Returns `st`, the call's status so far, or the failure to record.
static psk_soft_status front_release(const FrontCall &c, FrontPlan &plan, psk_soft_status st)
{
    const std::string keep = g_last_error;
    const hipError_t e1 = plan.sc->ev.record(c.stream), e2 = plan.ds->ev.record(c.stream);
    if (e1 != hipSuccess || e2 != hipSuccess) {
        (void)hipStreamSynchronize(c.stream);
        plan.ds->ev.clear();
        if (st == PSK_SOFT_OK)
            return fail(PSK_SOFT_ERR_HIP, std::string("hipEventRecord: ") + hipGetErrorString(e1 != hipSuccess ? e1 : e2));
    }
    g_last_error = keep;
    return st;
}

// 5. Commit: the histories the launches have written become the current ones -- only now that the whole call has succeeded.
static void front_commit(const FrontCall &c, const FrontPlan &plan)
{
    for (uint32_t i = 0; i < c.nch; i++) {
        if (plan.pkt[i].resample)
            c.h->rs_hist.flip(c.ch0 + i);
        if (plan.pkt[i].fir)
            c.h->fir_hist.flip(c.ch0 + i);
    }
}

// Strided packets (include/psk_soft_hip.h): every packet whose samples lie `sample_stride[i]` samples apart is gathered into a
// contiguous row of the gather scratch, in its own element type, on the caller's stream; a copy of the packet array points at the
// rows and the ordinary call runs on it.  process_round, the plans, the cut into pieces and every kernel behind it see contiguous
// packets.  Runs of packets that are adjacent columns of one frame-major matrix (frame groups, psk_gather.h) go through the tile
// kernel, the rest through the plain strided gather.
//
// Tuned packets (`tune` non-NULL and the packet's {phase, step} not {0, 0}), filtered packets (`fir` non-NULL and the packet's
// filter not 0) and resampled packets (`resample` non-NULL and the packet's step not 0) go through the same machinery: behind the
// gathers one launch each of the tune kernel (psk_tune.hip), the filter kernel (psk_fir.hip) and the resample kernel
// (psk_resample.hip) writes each of them as a float2 row of the same scratch -- shifted; tuned inside the same pass if it has a
// tune, filtered and decimated; tuned likewise, or read from the filter's row, and interpolated -- and the packet copy points at
// the last row with format CF32, its count and the scaled sri_xdelta.  The entries below with fewer arguments are this one with
// NULL for the rest.
psk_soft_status psk_soft_process_device_filtered(psk_soft_handle_t *h, uint32_t ch0, uint32_t nch, const psk_soft_packet_t *pkts,
                                                 const uint64_t *sample_stride, const psk_soft_tune_t *tune, const psk_soft_fir_t *fir,
                                                 const psk_soft_resample_t *resample, psk_soft_output_t *outs, void *stream_v)
{
    if (!sample_stride && !tune && !resample && !fir)
        return psk_soft_process_device(h, ch0, nch, pkts, outs, stream_v);
    if (!h || !pkts || !outs || !nch || (uint64_t)ch0 + nch > h->nch)
        return fail(PSK_SOFT_ERR_INVALID_ARG, "psk_soft_process: bad arguments");
    const FrontCall c = {h, ch0, nch, pkts, sample_stride, tune, fir, resample, stream_v ? (hipStream_t)stream_v : h->stream};
    FrontPlan plan;
    PSK_TRY(front_classify(c, plan));
    if (plan.nothing() || plan.unknown)
        return psk_soft_process_device(h, ch0, nch, pkts, outs, stream_v);
    std::vector<psk_soft_packet_t> pk;
    if (h->dry) {  // (a control-plane-only handle plans and counts)
        front_packets(c, plan, false, pk);
        return psk_soft_process_device(h, ch0, nch, pk.data(), outs, stream_v);
    }
    PSK_HIP(hipSetDevice(h->device));
    psk_soft_status st = front_enqueue(c, plan);
    if (!plan.owed)
        return st;
    if (st == PSK_SOFT_OK && !h->opt_diag_gather_only) {
        front_packets(c, plan, true, pk);
        st = psk_soft_process_device(h, ch0, nch, pk.data(), outs, stream_v);
    }
    st = front_release(c, plan, st);
    if (st == PSK_SOFT_OK)
        front_commit(c, plan);
    return st;
}

psk_soft_status psk_soft_process_device_resampled(psk_soft_handle_t *h, uint32_t ch0, uint32_t nch, const psk_soft_packet_t *pkts,
                                                  const uint64_t *sample_stride, const psk_soft_tune_t *tune,
                                                  const psk_soft_resample_t *resample, psk_soft_output_t *outs, void *stream_v)
{
    return psk_soft_process_device_filtered(h, ch0, nch, pkts, sample_stride, tune, nullptr, resample, outs, stream_v);
}

psk_soft_status psk_soft_process_device_tuned(psk_soft_handle_t *h, uint32_t ch0, uint32_t nch, const psk_soft_packet_t *pkts,
                                              const uint64_t *sample_stride, const psk_soft_tune_t *tune, psk_soft_output_t *outs,
                                              void *stream_v)
{
    return psk_soft_process_device_resampled(h, ch0, nch, pkts, sample_stride, tune, nullptr, outs, stream_v);
}

psk_soft_status psk_soft_process_device_strided(psk_soft_handle_t *h, uint32_t ch0, uint32_t nch, const psk_soft_packet_t *pkts,
                                                const uint64_t *sample_stride, psk_soft_output_t *outs, void *stream_v)
{
    return psk_soft_process_device_tuned(h, ch0, nch, pkts, sample_stride, nullptr, outs, stream_v);
}

// psk_soft_{resample,fir}_{get,set}_history behind their argument checks (a control-plane-only handle keeps zeros)
static psk_soft_status history_get(psk_soft_handle *h, HistoryBank &bank, uint32_t ch, float *out)
{
    if (!h->dry)
        PSK_HIP(hipSetDevice(h->device));
    return bank.get(ch, out);
}
static psk_soft_status history_set(psk_soft_handle *h, HistoryBank &bank, uint32_t ch, const float *in)
{
    if (h->dry)
        return PSK_SOFT_OK;
    PSK_HIP(hipSetDevice(h->device));
    return bank.set(h->nch, ch, in);
}

// ---- tuned packets: the host-side helpers (pure) ----
uint64_t psk_soft_tune_step(double cycles_per_sample)
{
    if (!std::isfinite(cycles_per_sample))
        return 0;
    const double r = cycles_per_sample - std::floor(cycles_per_sample);  // [0, 1]; 1 (a tiny negative rate) wraps to 0
    return r >= 1.0 ? 0 : (uint64_t)(r * 0x1p64);
}

uint64_t psk_soft_tune_advance(uint64_t phase, uint64_t step, uint64_t n_complex) { return phase + step * n_complex; }

psk_soft_status psk_soft_tune_apply(const psk_soft_tune_t *tune, const float *in, uint64_t n_complex, float *out)
{
    if (!tune || (n_complex && (!in || !out)))
        return fail(PSK_SOFT_ERR_INVALID_ARG, "psk_soft_tune_apply: null pointer");
    const float *const tab = psk::tune_tables();
    uint64_t p = tune->phase;
    for (uint64_t k = 0; k < n_complex; k++, p += tune->step) {
        const float xr = in[2u * k], xi = in[2u * k + 1u];  // (in == out is fine)
        psk::tune_rotate(tab, p, xr, xi, &out[2u * k], &out[2u * k + 1u]);
    }
    return PSK_SOFT_OK;
}

// ---- resampled packets: the host-side helpers (pure) ----
uint64_t psk_soft_resample_step(double in_per_out)
{
    if (!std::isfinite(in_per_out) || in_per_out < 0.5 || in_per_out > 2.0)
        return 0;
    return (uint64_t)(in_per_out * 0x1p32);
}

// (any n_complex: 128-bit arithmetic, so the helpers answer for lengths the entry refuses too)
uint64_t psk_soft_resample_count(const psk_soft_resample_t *rs, uint64_t n_complex)
{
    if (!rs || !rs->step)
        return n_complex;
    const unsigned __int128 end = (unsigned __int128)n_complex << 32;
    return rs->pos >= end ? 0u : (uint64_t)((end - rs->pos + rs->step - 1u) / rs->step);
}

uint64_t psk_soft_resample_advance(const psk_soft_resample_t *rs, uint64_t n_complex)
{
    if (!rs)
        return 0;
    if (!rs->step)
        return rs->pos;
    const unsigned __int128 end = (unsigned __int128)n_complex << 32;
    return (uint64_t)(rs->pos + (unsigned __int128)psk_soft_resample_count(rs, n_complex) * rs->step - end);
}

psk_soft_status psk_soft_resample_apply(const psk_soft_resample_t *rs, const float *hist_in, const float *in, uint64_t n_complex,
                                        float *out, float *hist_out)
{
    if (!rs || (n_complex && !in))
        return fail(PSK_SOFT_ERR_INVALID_ARG, "psk_soft_resample_apply: null pointer");
    if (rs->step < psk::kResampleStepMin || rs->step > psk::kResampleStepMax || rs->pos > psk::kResamplePosMax ||
        n_complex >= psk::kResampleMaxN || rs->pad || (rs->flags & ~(uint32_t)PSK_SOFT_RS_RESTART))
        return fail(PSK_SOFT_ERR_INVALID_ARG, "psk_soft_resample_apply: step outside [2^31, 2^33], pos above 2^33, 2^30 samples or more, pad or flags");
    const uint64_t n_out = psk::resample_count(rs->pos, rs->step, n_complex);
    if (n_out && !out)
        return fail(PSK_SOFT_ERR_INVALID_ARG, "psk_soft_resample_apply: null pointer");
    float hist[6] = {};
    if (hist_in && !(rs->flags & PSK_SOFT_RS_RESTART))
        std::memcpy(hist, hist_in, sizeof hist);
    // component q (0 re, 1 im) of s[j], j >= -3
    auto s = [&](int64_t j, int q) { return j < 0 ? hist[2 * (j + 3) + q] : in[2 * j + q]; };
    uint64_t t = rs->pos;
    for (uint64_t m = 0; m < n_out; m++, t += rs->step) {
        const int64_t i = (int64_t)(t >> 32);
        float w[4];
        psk::resample_taps((uint32_t)t, w);
        for (int q = 0; q < 2; q++) out[2u * m + q] = psk::resample_mix(w, s(i - 3, q), s(i - 2, q), s(i - 1, q), s(i, q));
    }
    if (hist_out) {
        float nh[6];
        for (int64_t j = 0; j < 3; j++)
            for (int q = 0; q < 2; q++) nh[2 * j + q] = s((int64_t)n_complex - 3 + j, q);
        std::memcpy(hist_out, nh, sizeof nh);
    }
    return PSK_SOFT_OK;
}

uint32_t psk_soft_resample_piece(void) { return psk::kResamplePiece; }

// the history of a channel: its current slot, behind the last resample launch
psk_soft_status psk_soft_resample_get_history(psk_soft_handle_t *h, uint32_t ch, float *out)
{
    if (!h || !out || ch >= h->nch)
        return fail(PSK_SOFT_ERR_INVALID_ARG, "psk_soft_resample_get_history: bad arguments");
    return history_get(h, h->rs_hist, ch, out);
}

psk_soft_status psk_soft_resample_set_history(psk_soft_handle_t *h, uint32_t ch, const float *in)
{
    if (!h || !in || ch >= h->nch)
        return fail(PSK_SOFT_ERR_INVALID_ARG, "psk_soft_resample_set_history: bad arguments");
    return history_set(h, h->rs_hist, ch, in);
}

// ---- filtered packets: the filters of a handle, the host-side helpers (pure) and the histories ----
psk_soft_status psk_soft_fir_define(psk_soft_handle_t *h, uint32_t slot, const float *taps, uint32_t n_taps)
{
    if (!h || !taps || slot >= psk::kFirSlots || !n_taps || n_taps > psk::kFirMaxTaps)
        return fail(PSK_SOFT_ERR_INVALID_ARG, "psk_soft_fir_define: null pointer, a slot above 63 or a tap count outside 1 .. 128");
    if (h->dry) {
        h->fir_ntaps[slot] = n_taps;  // (a control-plane-only handle checks and counts: the count is all it needs)
        return PSK_SOFT_OK;
    }
    PSK_HIP(hipSetDevice(h->device));
    if (!h->d_fir_taps)
        PSK_HIP(h->d_fir_taps.alloc((size_t)psk::kFirSlots * psk::kFirMaxTaps));
    PSK_TRY(h->fir_hist.wait());  // (no launch is still reading the slot)
    PSK_HIP(hipMemcpy(h->d_fir_taps + (size_t)psk::kFirMaxTaps * slot, taps, sizeof(float) * n_taps, hipMemcpyHostToDevice));
    h->fir_ntaps[slot] = n_taps;
    return PSK_SOFT_OK;
}

uint64_t psk_soft_fir_count(const psk_soft_fir_t *f, uint64_t n_complex)
{
    if (!f || !f->filter || !f->decim)
        return n_complex;
    return psk::fir_count(f->pos, f->decim, n_complex);
}

uint32_t psk_soft_fir_advance(const psk_soft_fir_t *f, uint64_t n_complex)
{
    if (!f)
        return 0;
    if (!f->filter || !f->decim)
        return f->pos;
    // (pos + n_out * D - n: below D; 128-bit arithmetic, so the helper answers for any length)
    return (uint32_t)((unsigned __int128)f->pos + (unsigned __int128)psk::fir_count(f->pos, f->decim, n_complex) * f->decim - n_complex);
}

psk_soft_status psk_soft_fir_apply(const psk_soft_fir_t *f, const float *taps, uint32_t n_taps, const float *hist_in, const float *in,
                                   uint64_t n_complex, float *out, float *hist_out)
{
    if (!f || !taps || (n_complex && !in))
        return fail(PSK_SOFT_ERR_INVALID_ARG, "psk_soft_fir_apply: null pointer");
    if (!n_taps || n_taps > psk::kFirMaxTaps || !f->decim || f->decim > psk::kFirMaxDecim || f->pos >= f->decim ||
        (f->flags & ~(uint32_t)PSK_SOFT_FIR_RESTART) || n_complex >= psk::kFirMaxN)
        return fail(PSK_SOFT_ERR_INVALID_ARG, "psk_soft_fir_apply: taps outside 1 .. 128, decim outside 1 .. 16, pos >= decim, flags, or 2^30 samples or more");
    const uint64_t n_out = psk::fir_count(f->pos, f->decim, n_complex);
    if (n_out && !out)
        return fail(PSK_SOFT_ERR_INVALID_ARG, "psk_soft_fir_apply: null pointer");
    float hist[2u * psk::kFirHist] = {};
    if (hist_in && !(f->flags & PSK_SOFT_FIR_RESTART))
        std::memcpy(hist, hist_in, sizeof hist);
    // component q (0 re, 1 im) of s[j], j >= -127
    auto s = [&](int64_t j, int q) { return j < 0 ? hist[2 * (j + (int64_t)psk::kFirHist) + q] : in[2 * j + q]; };
    for (uint64_t m = 0; m < n_out; m++) {
        const int64_t i = (int64_t)(f->pos + m * f->decim);
        for (int q = 0; q < 2; q++) {
            float acc = 0.0f;
            for (uint32_t j = 0; j < n_taps; j++) acc = psk::fir_step(j == 0, acc, taps[j], s(i - (int64_t)j, q));
            out[2u * m + q] = acc;
        }
    }
    if (hist_out) {
        float nh[2u * psk::kFirHist];
        for (int64_t j = 0; j < (int64_t)psk::kFirHist; j++)
            for (int q = 0; q < 2; q++) nh[2 * j + q] = s((int64_t)n_complex - (int64_t)psk::kFirHist + j, q);
        std::memcpy(hist_out, nh, sizeof nh);
    }
    return PSK_SOFT_OK;
}

uint32_t psk_soft_fir_piece(uint32_t decim) { return decim && decim <= psk::kFirMaxDecim ? psk::fir_piece(decim) : 0u; }

// the history of a channel: its current slot, behind the last filter launch
psk_soft_status psk_soft_fir_get_history(psk_soft_handle_t *h, uint32_t ch, float *out)
{
    if (!h || !out || ch >= h->nch)
        return fail(PSK_SOFT_ERR_INVALID_ARG, "psk_soft_fir_get_history: bad arguments");
    return history_get(h, h->fir_hist, ch, out);
}

psk_soft_status psk_soft_fir_set_history(psk_soft_handle_t *h, uint32_t ch, const float *in)
{
    if (!h || !in || ch >= h->nch)
        return fail(PSK_SOFT_ERR_INVALID_ARG, "psk_soft_fir_set_history: bad arguments");
    return history_set(h, h->fir_hist, ch, in);
}

// ---- psk_soft_acquire_device: the carrier offset of a packet (include/psk_soft_hip.h, psk_acquire.hip) ----
// One look at a packet per channel: the fold over pieces of kAcquirePiece samples and the join per packet, on the caller's stream,
// one record per covered channel.  Nothing of the control plane or of the demodulator's state is read but constelationSize, and
// nothing is written but the records (and, for the columns of a frame group, their rows of the gather scratch: front_layout).
// The entry is look_device with kAcquireLook; the pass goes through the reduction-pass layer (PassRing) as the quality pass's does.
// (a packet the call reads: present, complex data, at least one sample, a constellation the M-th power is defined for)
static bool acquire_looks_at(psk_soft_handle *h, uint32_t ch, const psk_soft_packet_t &k)
{
    const uint16_t M = ctl_of(h, ch).props.constelationSize;
    return k.present && k.sri_mode == 1 && k.n_floats >= 2 && (M == 2 || M == 4 || M == 8);
}

// What one look at a packet per channel is made of; look_device is the rest of psk_soft_acquire_device and psk_soft_symrate_device.
struct LookEntry {
    const StridedEntry &entry;  // its name and its message about alignment
    bool (*looks_at)(psk_soft_handle *h, uint32_t ch, const psk_soft_packet_t &k);    // a packet the call reads
    uint64_t (*n_used)(psk_soft_handle *h, uint32_t ch, uint64_t n);                   // ... and how many of its n samples
    void (*plan_record)(psk_soft_handle *h, uint32_t ch, const psk_soft_packet_t *k);  // the record of a control-plane-only handle
                                                                                       // (k: the packet if it is read, else nullptr)
    psk_soft_status (*enqueue)(const FrontCall &c, const FrontPlan &plan);             // the fold and the join
};

static psk_soft_status look_device(const LookEntry &e, psk_soft_handle_t *h, uint32_t ch0, uint32_t nch, const psk_soft_packet_t *pkts,
                                   const uint64_t *sample_stride, const psk_soft_tune_t *tune, void *stream_v)
{
    if (!h || !pkts || !nch || (uint64_t)ch0 + nch > h->nch)
        return fail(PSK_SOFT_ERR_INVALID_ARG, std::string(e.entry.name) + ": bad arguments");
    const FrontCall c = {h, ch0, nch, pkts, sample_stride, tune, nullptr, nullptr, stream_v ? (hipStream_t)stream_v : h->stream};
    auto looked_at = [&](uint32_t i) { return e.looks_at(h, ch0 + i, pkts[i]); };
    // the refusals, before anything is enqueued or any record changes
    for (uint32_t i = 0; i < nch; i++) {
        const psk_soft_packet_t &k = pkts[i];
        if (!k.present)
            continue;
        PSK_TRY(strided_refusal(e.entry, ch0 + i, k, c.stride(i), looked_at(i)));
        if (!psk::pkt_format_known(k.format)) {
            char buf[160];
            std::snprintf(buf, sizeof buf, "%s: channel %u: unknown packet format %u (PSK_SOFT_FORMAT_CF32 = 0, CS16 = 1, CS8 = 3, CF16 = 4)",
                          e.entry.name, ch0 + i, (unsigned)k.format);
            return fail(PSK_SOFT_ERR_INVALID_ARG, buf);
        }
        if (looked_at(i) && !k.data && !h->dry)
            return fail(PSK_SOFT_ERR_INVALID_ARG, e.entry.misaligned);
    }
    if (h->dry) {
        for (uint32_t i = 0; i < nch; i++) e.plan_record(h, ch0 + i, looked_at(i) ? &pkts[i] : nullptr);
        return PSK_SOFT_OK;
    }
    PSK_HIP(hipSetDevice(h->device));
    // strided packets: the columns of a frame group of at least kGatherMinGroup go through the tile gather into own-format rows of
    // the stream's gather scratch, which the fold reads; any other strided packet is read where it lies, at its stride.  A row
    // holds the samples the look uses, no more.
    FrontPlan plan;
    plan.singles_in_place = true;
    plan.pkt.assign(nch, FrontPkt{});
    for (uint32_t i = 0; i < nch; i++) {
        plan.pkt[i].gathered = c.stride(i) != 1 && looked_at(i);
        plan.pkt[i].n_in = pkts[i].n_floats / 2u;
        if (looked_at(i))
            plan.pkt[i].n_in = e.n_used(h, ch0 + i, plan.pkt[i].n_in);
    }
    psk_soft_status st = front_enqueue(c, plan);
    if (st == PSK_SOFT_OK)
        st = e.enqueue(c, plan);
    return plan.owed ? front_release(c, plan, st) : st;
}

static psk_soft_status acquire_enqueue(const FrontCall &c, const FrontPlan &plan);
static const LookEntry kAcquireLook = {
    kAcquireEntry, acquire_looks_at, [](psk_soft_handle *, uint32_t, uint64_t n) { return n; },
    [](psk_soft_handle *h, uint32_t ch, const psk_soft_packet_t *k) {
        psk_soft_acquire_t r = {};
        if (k) {
            r.n_samples = k->n_floats / 2u;
            r.constelationSize = ctl_of(h, ch).props.constelationSize;
            r.flags = PSK_SOFT_A_PLANNED;
        }
        h->acquire.dry[ch] = r;
    },
    acquire_enqueue};

psk_soft_status psk_soft_acquire_device(psk_soft_handle_t *h, uint32_t ch0, uint32_t nch, const psk_soft_packet_t *pkts,
                                        const uint64_t *sample_stride, const psk_soft_tune_t *tune, void *stream_v)
{
    return look_device(kAcquireLook, h, ch0, nch, pkts, sample_stride, tune, stream_v);
}

// the fold and the join of an acquire call whose arguments have passed (plan: the rows of its gathered packets)
static psk_soft_status acquire_enqueue(const FrontCall &c, const FrontPlan &plan)
{
    psk_soft_handle *const h = c.h;
    const uint32_t ch0 = c.ch0, nch = c.nch;
    const hipStream_t stream = c.stream;
    auto looked_at = [&](uint32_t i) { return acquire_looks_at(h, ch0 + i, c.pkts[i]); };
    auto &q = h->apass.next();
    PSK_TRY(h->apass.claim(q, h->nch));
    PieceCount parts;
    bool any_tuned = false;
    for (uint32_t i = 0; i < nch; i++) {
        psk::AcquireDesc &d = q.h_desc[i];
        d = psk::AcquireDesc{};
        d.channel = ch0 + i;
        if (!looked_at(i))
            continue;  // (its zero record)
        const psk_soft_packet_t &k = c.pkts[i];
        const void *const row = plan.pkt[i].own_row;
        d.src = row ? row : (const void *)k.data;
        d.stride = row ? 1u : c.stride(i);
        d.n = k.n_floats / 2u;
        d.M = ctl_of(h, ch0 + i).props.constelationSize;
        d.format = k.format;
        d.flags = PSK_SOFT_A_DATA;
        if (c.has_tune(i)) {
            d.phase = c.tune[i].phase, d.step = c.tune[i].step;
            d.flags |= PSK_SOFT_A_TUNED;
            any_tuned = true;
        }
        if (!parts.add((d.n + psk::kAcquirePiece - 1u) / psk::kAcquirePiece, &d.part0, &d.n_piece))
            return fail(PSK_SOFT_ERR_LIMIT, "psk_soft_acquire_device: too many samples in one call");
    }
    // (PSK_SOFT_TRACE_LAUNCHES, trace_launch: cnt = covered channels, tiles = pieces)
    auto mark = [&](const char *what) { return trace_launch(h, what, 0, 0, ch0, nch, parts.total, 0, 0, h->slot, stream); };
    return h->apass.run(q, nch, {ch0, nch}, parts.total, stream, [&]() -> psk_soft_status {
        if (any_tuned)
            PSK_TRY(ensure_tune_tab(h));
        PSK_HIP(mark("acquire_fold"));
        PSK_HIP(psk::launch_acquire_fold(q.d_desc, nch, parts.max_piece, any_tuned ? h->d_tune_tab : nullptr, q.d_part, stream));
        PSK_HIP(mark("acquire_join"));
        PSK_HIP(psk::launch_acquire_join(q.d_desc, nch, q.d_part, h->acquire.d, stream));
        return PSK_SOFT_OK;
    });
}

uint64_t psk_soft_acquire_bytes(void) { return sizeof(psk_soft_acquire_t); }
uint32_t psk_soft_acquire_piece(void) { return psk::kAcquirePiece; }

psk_soft_status psk_soft_get_acquire(psk_soft_handle_t *h, uint32_t ch0, uint32_t nch, psk_soft_acquire_t *rec)
{
    if (!h || !rec || !nch || (uint64_t)ch0 + nch > h->nch)
        return fail(PSK_SOFT_ERR_INVALID_ARG, "psk_soft_get_acquire: bad arguments");
    return records_read(h, h->acquire, h->apass, ch0, nch, rec);
}

psk_soft_status psk_soft_acquire_host(uint16_t constelationSize, const psk_soft_tune_t *tune, const float *in, uint64_t n_complex,
                                      psk_soft_acquire_t *rec)
{
    const uint16_t M = constelationSize;
    if (!rec || (n_complex && !in) || !(M == 2 || M == 4 || M == 8))
        return fail(PSK_SOFT_ERR_INVALID_ARG, "psk_soft_acquire_host: null pointer, or a constelationSize other than 2, 4, 8");
    *rec = psk_soft_acquire_t{};
    if (!n_complex)
        return PSK_SOFT_OK;  // (no sample: the zero record)
    const bool tuned = tune && (tune->phase | tune->step) != 0;
    const float *const tab = tuned ? psk::tune_tables() : nullptr;
    const int P = M == 2 ? 1 : M == 4 ? 2 : 3;
    // the phasors of the last kAcquireHalo samples, by index mod kAcquireHalo
    float ur[psk::kAcquireHalo], ui[psk::kAcquireHalo];
    bool valid[psk::kAcquireHalo];
    uint64_t p = tuned ? tune->phase : 0;
    for (uint64_t k = 0; k < n_complex; k++) {
        float re = in[2u * k], im = in[2u * k + 1u];
        if (tuned) {
            psk::tune_rotate(tab, p, re, im, &re, &im);
            p += tune->step;
        }
        float e, r, i;
        const bool ok = psk::acq_sample(re, im, P, &e, &r, &i);
        if (ok) {
            rec->sum_e += (double)e;
            rec->n_valid++;
            for (uint32_t j = 0; j < psk::kAcquireLags; j++) {
                const uint64_t L = (uint64_t)1 << j;
                if (k < L)
                    break;
                if (!valid[(k - L) % psk::kAcquireHalo])
                    continue;
                const float vr = ur[(k - L) % psk::kAcquireHalo], vi = ui[(k - L) % psk::kAcquireHalo];
                float tr, ti;
                psk::acq_lag(r, i, vr, vi, &tr, &ti);
                rec->sum_re[j] += (double)tr;
                rec->sum_im[j] += (double)ti;
                rec->n_pairs[j]++;
            }
        }
        ur[k % psk::kAcquireHalo] = r, ui[k % psk::kAcquireHalo] = i, valid[k % psk::kAcquireHalo] = ok;
    }
    rec->n_samples = n_complex;
    rec->constelationSize = M;
    rec->flags = (uint8_t)(PSK_SOFT_A_DATA | (tuned ? PSK_SOFT_A_TUNED : 0));
    return PSK_SOFT_OK;
}

psk_soft_status psk_soft_acquire_derive(const psk_soft_acquire_t *rec, psk_soft_acquire_derived_t *d)
{
    if (!rec || !d)
        return fail(PSK_SOFT_ERR_INVALID_ARG, "psk_soft_acquire_derive: null pointer");
    const double nan = std::nan(""), two_pi = 2.0 * 3.14159265358979323846;
    *d = psk_soft_acquire_derived_t{};
    d->offset_cycles_per_sample = d->coherence = d->mean_energy = nan;
    if (!(rec->flags & PSK_SOFT_A_DATA) || !rec->n_pairs[0] || (rec->sum_re[0] == 0.0 && rec->sum_im[0] == 0.0))
        return PSK_SOFT_OK;
    const double M = (double)rec->constelationSize;
    const double c0 = std::hypot(rec->sum_re[0], rec->sum_im[0]) / (double)rec->n_pairs[0];
    double f = std::atan2(rec->sum_im[0], rec->sum_re[0]) / (two_pi * M);
    int32_t used = 1;
    for (uint32_t j = 1; j < psk::kAcquireLags; j++) {
        if (!rec->n_pairs[j])
            break;
        const double cj = std::hypot(rec->sum_re[j], rec->sum_im[j]) / (double)rec->n_pairs[j];
        if (cj < 0.5 * c0)
            break;
        const double L = (double)(1u << j);
        double dd = std::atan2(rec->sum_im[j], rec->sum_re[j]) - two_pi * M * L * f;
        dd -= two_pi * std::rint(dd / two_pi);
        f += dd / (two_pi * M * L);
        used++;
    }
    d->offset_cycles_per_sample = f;
    d->coherence = c0;
    d->mean_energy = rec->n_valid ? rec->sum_e / (double)rec->n_valid : nan;
    d->lags_used = used;
    return PSK_SOFT_OK;
}

// ---- psk_soft_symrate_device: the symbol rate of a packet (include/psk_soft_hip.h, psk_symrate.hip) ----
// The second look (look_device, kSymrateLook): a fold over pieces of kSymratePiece blocks and a join per packet on the caller's
// stream, one record per covered channel; the gather takes the samples the look uses, no more; a pass ring of its own.  Nothing of the
// control plane is read but samplesPerBaud, nothing is written but the records and the rows of the gather scratch.
// (a packet the call reads: present, complex data, a block length the look is defined for, at least two blocks)
static bool symrate_looks_at(psk_soft_handle *h, uint32_t ch, const psk_soft_packet_t &k)
{
    const uint32_t S = ctl_of(h, ch).props.samplesPerBaud;
    return k.present && k.sri_mode == 1 && S >= psk::kSymrateMinS && S <= psk::kSymrateMaxS && k.n_floats / 2u >= 2u * (uint64_t)S;
}
// blocks the look uses of n samples
static uint32_t symrate_blocks(uint64_t n, uint32_t S)
{
    const uint64_t b = n / S;
    return (uint32_t)(b < psk::kSymrateMaxBlocks ? b : psk::kSymrateMaxBlocks);
}

static const StridedEntry kSymrateEntry = {"psk_soft_symrate_device", "psk_soft_symrate_device: packet data must be 8-byte aligned (CS16: 4) (CS8: 2) (CF16: 4)"};
static psk_soft_status symrate_enqueue(const FrontCall &c, const FrontPlan &plan);
static const LookEntry kSymrateLook = {
    kSymrateEntry, symrate_looks_at,
    [](psk_soft_handle *h, uint32_t ch, uint64_t n) {
        const uint32_t S = ctl_of(h, ch).props.samplesPerBaud;
        return (uint64_t)symrate_blocks(n, S) * S;
    },
    [](psk_soft_handle *h, uint32_t ch, const psk_soft_packet_t *k) {
        psk_soft_symrate_t r = {};
        if (k) {
            const uint32_t S = ctl_of(h, ch).props.samplesPerBaud;
            r.n_samples = k->n_floats / 2u;
            r.n_blocks = symrate_blocks(r.n_samples, S);
            r.n_used = r.n_blocks * S;
            r.samplesPerBaud = (uint16_t)S;
            r.flags = PSK_SOFT_SR_PLANNED;
        }
        h->symrate.dry[ch] = r;
    },
    symrate_enqueue};

psk_soft_status psk_soft_symrate_device(psk_soft_handle_t *h, uint32_t ch0, uint32_t nch, const psk_soft_packet_t *pkts,
                                        const uint64_t *sample_stride, const psk_soft_tune_t *tune, void *stream_v)
{
    return look_device(kSymrateLook, h, ch0, nch, pkts, sample_stride, tune, stream_v);
}

// the fold and the join of a symbol-rate call whose arguments have passed (plan: the rows of its gathered packets)
static psk_soft_status symrate_enqueue(const FrontCall &c, const FrontPlan &plan)
{
    psk_soft_handle *const h = c.h;
    const uint32_t ch0 = c.ch0, nch = c.nch;
    const hipStream_t stream = c.stream;
    auto &q = h->spass.next();
    PSK_TRY(h->spass.claim(q, h->nch));
    PieceCount parts;
    for (uint32_t i = 0; i < nch; i++) {
        psk::SymrateDesc &d = q.h_desc[i];
        d = psk::SymrateDesc{};
        d.channel = ch0 + i;
        if (!symrate_looks_at(h, ch0 + i, c.pkts[i]))
            continue;  // (its zero record)
        const psk_soft_packet_t &k = c.pkts[i];
        const void *const row = plan.pkt[i].own_row;
        d.src = row ? row : (const void *)k.data;
        d.stride = row ? 1u : c.stride(i);
        d.n = k.n_floats / 2u;
        d.S = ctl_of(h, ch0 + i).props.samplesPerBaud;
        d.wstep = psk::sr_wstep(d.S);
        d.n_blocks = symrate_blocks(d.n, d.S);
        d.format = k.format;
        d.flags = PSK_SOFT_SR_DATA;
        if (c.has_tune(i)) {
            d.phase = c.tune[i].phase, d.step = c.tune[i].step;
            d.flags |= PSK_SOFT_SR_TUNED;
        }
        // (at most 8 pieces a packet: the count cannot refuse)
        (void)parts.add((d.n_blocks + psk::kSymratePiece - 1u) / psk::kSymratePiece, &d.part0, &d.n_piece);
    }
    // (PSK_SOFT_TRACE_LAUNCHES, trace_launch: cnt = covered channels, tiles = pieces)
    auto mark = [&](const char *what) { return trace_launch(h, what, 0, 0, ch0, nch, parts.total, 0, 0, h->slot, stream); };
    return h->spass.run(q, nch, {ch0, nch}, parts.total, stream, [&]() -> psk_soft_status {
        PSK_TRY(ensure_tune_tab(h));  // (the block phasors come from the tables, tuned or not)
        PSK_HIP(mark("symrate_fold"));
        PSK_HIP(psk::launch_symrate_fold(q.d_desc, nch, parts.max_piece, h->d_tune_tab, q.d_part, stream));
        PSK_HIP(mark("symrate_join"));
        PSK_HIP(psk::launch_symrate_join(q.d_desc, nch, q.d_part, h->symrate.d, stream));
        return PSK_SOFT_OK;
    });
}

uint64_t psk_soft_symrate_bytes(void) { return sizeof(psk_soft_symrate_t); }
uint32_t psk_soft_symrate_piece(void) { return psk::kSymratePiece; }

psk_soft_status psk_soft_get_symrate(psk_soft_handle_t *h, uint32_t ch0, uint32_t nch, psk_soft_symrate_t *rec)
{
    if (!h || !rec || !nch || (uint64_t)ch0 + nch > h->nch)
        return fail(PSK_SOFT_ERR_INVALID_ARG, "psk_soft_get_symrate: bad arguments");
    return records_read(h, h->symrate, h->spass, ch0, nch, rec);
}

psk_soft_status psk_soft_symrate_host(uint16_t samplesPerBaud, const psk_soft_tune_t *tune, const float *in, uint64_t n_complex,
                                      psk_soft_symrate_t *rec)
{
    const uint32_t S = samplesPerBaud;
    if (!rec || (n_complex && !in) || S < psk::kSymrateMinS || S > psk::kSymrateMaxS)
        return fail(PSK_SOFT_ERR_INVALID_ARG, "psk_soft_symrate_host: null pointer, or a samplesPerBaud outside 4 .. 1024");
    *rec = psk_soft_symrate_t{};
    if (n_complex < 2u * (uint64_t)S)
        return PSK_SOFT_OK;  // (fewer than two blocks: the zero record)
    const bool tuned = tune && (tune->phase | tune->step) != 0;
    const float *const tab = psk::tune_tables();
    const uint64_t wstep = psk::sr_wstep(S);
    const uint32_t n_blocks = symrate_blocks(n_complex, S);
    // the sums of the last kSymrateHalo blocks, by index mod kSymrateHalo: B_e (re, im), B_g (re, im)
    double B[psk::kSymrateHalo][4];
    bool valid[psk::kSymrateHalo];
    uint64_t ph = tuned ? tune->phase : 0;
    float pre = 0.0f, pim = 0.0f;
    for (uint32_t m = 0; m < n_blocks; m++) {
        double a[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
        bool ok = true;
        for (uint32_t p = 0; p < S; p++) {
            const uint64_t k = (uint64_t)m * S + p;
            float re = in[2u * k], im = in[2u * k + 1u];
            if (tuned) {
                psk::tune_rotate(tab, ph, re, im, &re, &im);
                ph += tune->step;
            }
            float e, g, cs, sn, tr, ti;
            ok = psk::sr_sample(re, im, pre, pim, k != 0, &e, &g) && ok;
            psk::tune_phasor(tab, psk::sr_phase(p, wstep), &cs, &sn);
            psk::sr_term(e, cs, sn, &tr, &ti);
            a[0] += (double)tr, a[1] += (double)ti;
            psk::sr_term(g, cs, sn, &tr, &ti);
            a[2] += (double)tr, a[3] += (double)ti;
            a[4] += (double)e, a[5] += (double)g;
            pre = re, pim = im;
        }
        if (ok) {
        rec->n_valid++;
        rec->sum_pow[0] += psk::sr_pow(a[0], a[1]), rec->sum_pow[1] += psk::sr_pow(a[2], a[3]);
        rec->sum_lvl[0] += a[4], rec->sum_lvl[1] += a[5];
        for (uint32_t j = 0; j < psk::kSymrateLags; j++) {
            const uint32_t L = 1u << j;
            if (m < L)
                break;
            if (!valid[(m - L) % psk::kSymrateHalo])
                continue;
            const double *const o = B[(m - L) % psk::kSymrateHalo];
            double tr, ti;
            psk::sr_lag(a[0], a[1], o[0], o[1], &tr, &ti);
            rec->sum_re[0][j] += tr, rec->sum_im[0][j] += ti;
            psk::sr_lag(a[2], a[3], o[2], o[3], &tr, &ti);
            rec->sum_re[1][j] += tr, rec->sum_im[1][j] += ti;
            rec->n_pairs[j]++;
        }
        }
        // (behind the lags: lag 128 reads the slot this block takes)
        double *const b = B[m % psk::kSymrateHalo];
        b[0] = a[0], b[1] = a[1], b[2] = a[2], b[3] = a[3];
        valid[m % psk::kSymrateHalo] = ok;
    }
    rec->n_samples = n_complex;
    rec->n_blocks = n_blocks;
    rec->n_used = (uint64_t)n_blocks * S;
    rec->samplesPerBaud = samplesPerBaud;
    rec->flags = (uint8_t)(PSK_SOFT_SR_DATA | (tuned ? PSK_SOFT_SR_TUNED : 0));
    return PSK_SOFT_OK;
}

psk_soft_status psk_soft_symrate_derive(const psk_soft_symrate_t *rec, psk_soft_symrate_derived_t *d)
{
    if (!rec || !d)
        return fail(PSK_SOFT_ERR_INVALID_ARG, "psk_soft_symrate_derive: null pointer");
    const double nan = std::nan(""), two_pi = 2.0 * 3.14159265358979323846;
    *d = psk_soft_symrate_derived_t{};
    d->samples_per_symbol = d->step_ratio = d->coherence = d->mean_level = nan;
    d->detector = -1;
    if (!(rec->flags & PSK_SOFT_SR_DATA) || !rec->n_pairs[0] || !rec->n_valid)
        return PSK_SOFT_OK;
    // c_j of detector z
    auto coh = [&](int z, uint32_t j) {
        return std::hypot(rec->sum_re[z][j], rec->sum_im[z][j]) / ((double)rec->n_pairs[j] * (rec->sum_pow[z] / (double)rec->n_valid));
    };
    double c0[2];
    for (int z = 0; z < 2; z++) c0[z] = rec->sum_re[z][0] == 0.0 && rec->sum_im[z][0] == 0.0 ? 0.0 : coh(z, 0);
    if (c0[0] == 0.0 && c0[1] == 0.0)
        return PSK_SOFT_OK;
    const int z = c0[1] > c0[0] ? 1 : 0;
    double f = std::atan2(rec->sum_im[z][0], rec->sum_re[z][0]) / two_pi;
    int32_t used = 1;
    for (uint32_t j = 1; j < psk::kSymrateLags; j++) {
        if (rec->n_pairs[j] < 8u || coh(z, j) < 0.5 * c0[z])
            break;
        const double L = (double)(1u << j);
        double dd = std::atan2(rec->sum_im[z][j], rec->sum_re[z][j]) - two_pi * L * f;
        dd -= two_pi * std::rint(dd / two_pi);
        f += dd / (two_pi * L);
        used++;
    }
    d->samples_per_symbol = (double)rec->samplesPerBaud / (1.0 + f);
    d->step_ratio = 1.0 / (1.0 + f);
    d->coherence = c0[z];
    d->mean_level = rec->sum_lvl[z] / ((double)rec->n_valid * (double)rec->samplesPerBaud);
    d->detector = z;
    d->lags_used = used;
    return PSK_SOFT_OK;
}

// ---- psk_soft_sync_device: a known word in the soft symbols (include/psk_soft_hip.h, psk_sync.hip) ----
// The second reduction behind a call, after the quality pass: a fold over pieces of kSyncPiece windows and a join per channel on
// the caller's stream, one record per covered channel; a pass ring of its own, a history bank like the filter's.  Nothing of the
// control plane or of the demodulator's state is read, nothing is written but the records and the histories.
psk_soft_status psk_soft_sync_define(psk_soft_handle_t *h, uint32_t slot, const float *word, uint32_t n)
{
    if (!h || !word || slot >= psk::kSyncSlots || !n || n > psk::kSyncMaxWord)
        return fail(PSK_SOFT_ERR_INVALID_ARG, "psk_soft_sync_define: null pointer, a slot above 15 or a word length outside 1 .. 128");
    if (!h->dry) {
        PSK_HIP(hipSetDevice(h->device));
        if (!h->d_sync_words)
            PSK_HIP(h->d_sync_words.alloc((size_t)2u * psk::kSyncSlots * psk::kSyncMaxWord));
        PSK_TRY(h->sync_hist.wait());  // (no launch is still reading the slot)
        PSK_HIP(hipMemcpy(h->d_sync_words + (size_t)2u * psk::kSyncMaxWord * slot, word, sizeof(float) * 2u * n, hipMemcpyHostToDevice));
        h->sync_ew[slot] = psk::sy_word_energy(word, n);
    }
    h->sync_len[slot] = n;  // (a control-plane-only handle checks and counts: the length is all it needs)
    return PSK_SOFT_OK;
}

// a channel the call searches
static bool sync_searched(const psk_soft_sync_in_t &k) { return k.word != 0u && k.soft != nullptr && k.n_symbols != 0u; }
static bool sync_threshold_ok(float t) { return t > 0.0f && t <= 1.0f; }  // (false for NaN)

static psk_soft_status sync_enqueue(psk_soft_handle *h, uint32_t ch0, uint32_t nch, const psk_soft_sync_in_t *in, hipStream_t stream);

// how a call that went through leaves its covered channels for PSK_SOFT_DEMAP_FRONT: searched or not, and with which flags
static void sync_remember(psk_soft_handle *h, uint32_t ch0, uint32_t nch, const psk_soft_sync_in_t *in)
{
    if (h->sync_last.empty())
        h->sync_last.assign(h->nch, psk_soft_handle::kSyncNotSearched);
    for (uint32_t i = 0; i < nch; i++)
        h->sync_last[ch0 + i] = !sync_searched(in[i])                      ? psk_soft_handle::kSyncNotSearched
                                : (in[i].flags & PSK_SOFT_SYNC_RESTART) ? psk_soft_handle::kSyncSearchedRestart
                                                                        : psk_soft_handle::kSyncSearched;
}

psk_soft_status psk_soft_sync_device(psk_soft_handle_t *h, uint32_t ch0, uint32_t nch, const psk_soft_sync_in_t *in, void *stream_v)
{
    if (!h || !in || !nch || (uint64_t)ch0 + nch > h->nch)
        return fail(PSK_SOFT_ERR_INVALID_ARG, "psk_soft_sync_device: bad arguments");
    // the refusals, before anything is enqueued, any record changes or any history flips
    for (uint32_t i = 0; i < nch; i++) {
        const psk_soft_sync_in_t &k = in[i];
        if (!sync_searched(k))
            continue;
        const char *what = nullptr;
        if (k.word > psk::kSyncSlots || !h->sync_len[k.word - 1u])
            what = "a word slot above 15 or never defined (psk_soft_sync_define)";
        else if (!sync_threshold_ok(k.threshold))
            what = "a threshold that is NaN, <= 0 or > 1";
        else if (k.flags & ~(uint32_t)PSK_SOFT_SYNC_RESTART)
            what = "unknown flag bits";
        else if (k.pad)
            what = "pad must be zero";
        else if ((uintptr_t)k.soft & 7u)
            what = "soft must be 8-byte aligned";
        else if (k.n_symbols >= psk::kSyncMaxN)
            what = "2^30 symbols or more";
        if (what) {
            char buf[160];
            std::snprintf(buf, sizeof buf, "psk_soft_sync_device: channel %u: %s", ch0 + i, what);
            return fail(PSK_SOFT_ERR_INVALID_ARG, buf);
        }
    }
    PSK_TRY(h->sync.ensure_zeroed(h->dry, h->nch, "sync records"));  // (zeros until a call writes one)
    if (h->dry) {
        for (uint32_t i = 0; i < nch; i++) {
            psk_soft_sync_t r = {};
            if (sync_searched(in[i])) {
                int64_t p0;
                r.word_len = h->sync_len[in[i].word - 1u];
                r.n_symbols = in[i].n_symbols;
                r.n_windows = psk::sync_windows(in[i].n_symbols, r.word_len, (in[i].flags & PSK_SOFT_SYNC_RESTART) != 0, &p0);
                r.flags = PSK_SOFT_SYNC_PLANNED;
            }
            h->sync.dry[ch0 + i] = r;
        }
        sync_remember(h, ch0, nch, in);
        return PSK_SOFT_OK;
    }
    PSK_HIP(hipSetDevice(h->device));
    hipStream_t stream = stream_v ? (hipStream_t)stream_v : h->stream;
    // (a deferred call's classes end on the side streams: the rows must be complete)
    PSK_HIP(deferred_join(h, stream));
    PSK_TRY(h->sync_hist.ensure(h->nch));
    const psk_soft_status st = sync_enqueue(h, ch0, nch, in, stream);
    if (st != PSK_SOFT_OK && !h->sync_last.empty())  // (a launch may have written the other slots: nothing for FRONT to read there)
        for (uint32_t i = 0; i < nch; i++) h->sync_last[ch0 + i] = psk_soft_handle::kSyncNotSearched;
    if (st == PSK_SOFT_OK) {  // (the whole call went through: the new histories are the channels')
        for (uint32_t i = 0; i < nch; i++)
            if (sync_searched(in[i]))
                h->sync_hist.flip(ch0 + i);
        sync_remember(h, ch0, nch, in);
    }
    return st;
}

// the fold and the join of a sync call whose arguments have passed
static psk_soft_status sync_enqueue(psk_soft_handle *h, uint32_t ch0, uint32_t nch, const psk_soft_sync_in_t *in, hipStream_t stream)
{
    auto &q = h->ypass.next();
    PSK_TRY(h->ypass.claim(q, h->nch));
    PieceCount parts;
    for (uint32_t i = 0; i < nch; i++) {
        psk::SyncDesc &d = q.h_desc[i];
        d = psk::SyncDesc{};
        d.channel = ch0 + i;
        const psk_soft_sync_in_t &k = in[i];
        if (!sync_searched(k))
            continue;  // (its zero record; the history stays)
        const uint32_t slot = k.word - 1u;
        const bool restart = (k.flags & PSK_SOFT_SYNC_RESTART) != 0;
        d.soft = k.soft;
        d.word = h->d_sync_words + (size_t)2u * psk::kSyncMaxWord * slot;
        d.hist_in = h->sync_hist.in(ch0 + i), d.hist_out = h->sync_hist.out(ch0 + i);
        d.n = k.n_symbols;
        d.L = h->sync_len[slot];
        d.n_windows = psk::sync_windows(d.n, d.L, restart, &d.p0);
        d.flags = psk::kSyncData | (restart ? psk::kSyncRestart : 0u);
        d.threshold = k.threshold, d.Ew = h->sync_ew[slot];
        // (a row without a window still has a piece: its workgroup writes the history)
        if (!parts.add(d.n_windows ? (d.n_windows + psk::kSyncPiece - 1u) / psk::kSyncPiece : 1u, &d.part0, &d.n_piece))
            return fail(PSK_SOFT_ERR_LIMIT, "psk_soft_sync_device: too many symbols in one call");
    }
    // (PSK_SOFT_TRACE_LAUNCHES, trace_launch: cnt = covered channels, tiles = pieces)
    auto mark = [&](const char *what) { return trace_launch(h, what, 0, 0, ch0, nch, parts.total, 0, 0, h->slot, stream); };
    return h->ypass.run(q, nch, {ch0, nch}, parts.total, stream, [&]() -> psk_soft_status {
        PSK_HIP(mark("sync_fold"));
        PSK_HIP(psk::launch_sync_fold(q.d_desc, nch, parts.max_piece, q.d_part, stream));
        PSK_HIP(mark("sync_join"));
        PSK_HIP(psk::launch_sync_join(q.d_desc, nch, q.d_part, h->sync.d, stream));
        PSK_TRY(h->sync_hist.record(stream));
        return PSK_SOFT_OK;
    });
}

uint64_t psk_soft_sync_bytes(void) { return sizeof(psk_soft_sync_t); }
uint64_t psk_soft_sync_in_bytes(void) { return sizeof(psk_soft_sync_in_t); }
uint32_t psk_soft_sync_piece(void) { return psk::kSyncPiece; }
static_assert(sizeof(psk_soft_sync_t) == 456 && sizeof(psk_soft_sync_in_t) == 32 && sizeof(psk_soft_sync_hit_t) == 24, "include/psk_soft_hip.h states the sizes");

psk_soft_status psk_soft_get_sync(psk_soft_handle_t *h, uint32_t ch0, uint32_t nch, psk_soft_sync_t *rec)
{
    if (!h || !rec || !nch || (uint64_t)ch0 + nch > h->nch)
        return fail(PSK_SOFT_ERR_INVALID_ARG, "psk_soft_get_sync: bad arguments");
    if (!h->sync.exist()) {  // (no call yet: the records are zeros)
        std::memset(rec, 0, sizeof(psk_soft_sync_t) * nch);
        return PSK_SOFT_OK;
    }
    return records_read(h, h->sync, h->ypass, ch0, nch, rec);
}

// the history of a channel: its current slot, behind the last sync launch
psk_soft_status psk_soft_sync_get_history(psk_soft_handle_t *h, uint32_t ch, float *out)
{
    if (!h || !out || ch >= h->nch)
        return fail(PSK_SOFT_ERR_INVALID_ARG, "psk_soft_sync_get_history: bad arguments");
    return history_get(h, h->sync_hist, ch, out);
}

psk_soft_status psk_soft_sync_set_history(psk_soft_handle_t *h, uint32_t ch, const float *in)
{
    if (!h || !in || ch >= h->nch)
        return fail(PSK_SOFT_ERR_INVALID_ARG, "psk_soft_sync_set_history: bad arguments");
    return history_set(h, h->sync_hist, ch, in);
}

psk_soft_status psk_soft_sync_host(const float *word, uint32_t L, float threshold, uint32_t flags, const float *hist_in, const float *soft,
                                   uint64_t n, psk_soft_sync_t *rec, float *hist_out)
{
    if (!word || !rec || (n && !soft))
        return fail(PSK_SOFT_ERR_INVALID_ARG, "psk_soft_sync_host: null pointer");
    if (!L || L > psk::kSyncMaxWord || !sync_threshold_ok(threshold) || (flags & ~(uint32_t)PSK_SOFT_SYNC_RESTART) || n >= psk::kSyncMaxN)
        return fail(PSK_SOFT_ERR_INVALID_ARG, "psk_soft_sync_host: a word length outside 1 .. 128, a threshold that is NaN, <= 0 or > 1, flags, or 2^30 symbols or more");
    *rec = psk_soft_sync_t{};
    const bool restart = (flags & PSK_SOFT_SYNC_RESTART) != 0;
    float hist[2u * psk::kSyncHist] = {};
    if (hist_in && !(restart && n))  // (a row without symbols is not searched: its history does not move)
        std::memcpy(hist, hist_in, sizeof hist);
    if (!n) {
        if (hist_out)
            std::memcpy(hist_out, hist, sizeof hist);
        return PSK_SOFT_OK;
    }
    // component c (0 re, 1 im) of x[g], g >= -127
    auto x = [&](int64_t g, int c) { return g < 0 ? hist[2 * (g + (int64_t)psk::kSyncHist) + c] : soft[2 * g + c]; };
    const float Ew = psk::sy_word_energy(word, L);
    int64_t p0;
    rec->n_symbols = n;
    rec->n_windows = psk::sync_windows(n, L, restart, &p0);
    rec->word_len = L, rec->flags = PSK_SOFT_SYNC_DATA;
    bool has_best = false;
    for (uint64_t k = 0; k < rec->n_windows; k++) {
        const int64_t p = p0 + (int64_t)k;
        float cr = 0.0f, ci = 0.0f, e = 0.0f, m;
        for (uint32_t j = 0; j < L; j++) {
            const float xr = x(p + j, 0), xi = x(p + j, 1);
            psk::sy_step(j == 0, xr, xi, psk::sy_energy(xr, xi), word[2u * j], word[2u * j + 1u], &cr, &ci, &e);
        }
        if (!psk::sy_metric(cr, ci, e, Ew, &m))
            continue;
        rec->n_valid++;
        psk_soft_sync_hit_t hit = {};
        hit.pos = p, hit.cr = cr, hit.ci = ci, hit.e = e, hit.m = m;
        if (!has_best || m > rec->best.m)
            rec->best = hit, has_best = true;
        if (m >= threshold) {
            if (rec->n_hits < psk::kSyncHits)
                rec->hits[rec->n_hits] = hit;
            rec->n_hits++;
        }
    }
    if (hist_out) {
        float nh[2u * psk::kSyncHist];
        for (int64_t j = 0; j < (int64_t)psk::kSyncHist; j++)
            for (int c = 0; c < 2; c++) nh[2 * j + c] = x((int64_t)n - (int64_t)psk::kSyncHist + j, c);
        std::memcpy(hist_out, nh, sizeof nh);
    }
    return PSK_SOFT_OK;
}

psk_soft_status psk_soft_sync_derive(const psk_soft_sync_hit_t *hit, uint16_t constelationSize, uint32_t word_len, float Ew,
                                     psk_soft_sync_derived_t *out)
{
    const uint32_t M = constelationSize;
    if (!hit || !out || (M != 2 && M != 4 && M != 8) || !word_len || word_len > psk::kSyncMaxWord)
        return fail(PSK_SOFT_ERR_INVALID_ARG, "psk_soft_sync_derive: null pointer, a constelationSize other than 2, 4, 8 or a word length outside 1 .. 128");
    const double nan = std::nan(""), two_pi = 2.0 * 3.14159265358979323846;
    *out = psk_soft_sync_derived_t{};
    out->angle = out->residual = out->amplitude = out->metric = nan;
    out->rotation = -1;
    const psk_soft_sync_hit_t zero = {};
    if (!std::memcmp(hit, &zero, sizeof zero))
        return PSK_SOFT_OK;
    const double cr = hit->cr, ci = hit->ci, e = hit->e;
    const double angle = std::atan2(ci, cr), turns = std::rint(angle * M / two_pi);
    out->angle = angle;
    out->rotation = (int32_t)(((int64_t)turns % (int64_t)M + (int64_t)M) % (int64_t)M);
    out->residual = angle - turns * two_pi / M;
    out->amplitude = std::sqrt(e / (double)word_len);
    out->metric = (cr * cr + ci * ci) / (e * (double)Ew);
    return PSK_SOFT_OK;
}

// ---- psk_soft_demap_device: segments of the soft rows as per-bit LLRs (include/psk_soft_hip.h, psk_demap.hip) ----
// Behind the sync call: a fold over pieces of kDemapPiece symbols and a join per segment on the caller's stream, one record per
// segment of the call; a ring of its own, two slots whose descriptors grow on demand (up to 2^20 segments a call).  Nothing of the
// control plane, of the demodulator's state or of any other record is read or written; of the sync pass only the history slot its
// last call read.
static bool demap_map_ok(uint32_t M, const float *points, const uint8_t *labels)
{
    if (M != 2u && M != 4u && M != 8u)
        return false;
    uint32_t seen = 0;
    for (uint32_t k = 0; k < M; k++) {
        if (!psk::dm_finite(points[2u * k]) || !psk::dm_finite(points[2u * k + 1u]) || labels[k] >= M)
            return false;
        seen |= 1u << labels[k];
    }
    return seen == (1u << M) - 1u;
}

static psk::DemapMap demap_map_make(uint32_t M, const float *points, const uint8_t *labels)
{
    psk::DemapMap m = {};
    m.M = M, m.B = M == 2u ? 1u : M == 4u ? 2u : 3u;
    for (uint32_t k = 0; k < M; k++) m.p[2u * k] = points[2u * k], m.p[2u * k + 1u] = points[2u * k + 1u], m.label[k] = labels[k];
    return m;
}

psk_soft_status psk_soft_demap_define(psk_soft_handle_t *h, uint32_t slot, uint32_t M, const float *points, const uint8_t *labels)
{
    if (!h || !points || !labels || slot >= psk::kDemapSlots || !demap_map_ok(M, points, labels))
        return fail(PSK_SOFT_ERR_INVALID_ARG, "psk_soft_demap_define: null pointer, a slot above 15, an M other than 2, 4, 8, a non-finite point or labels that are not a permutation of 0 .. M-1");
    if (!h->dry) {
        PSK_HIP(hipSetDevice(h->device));
        if (!h->d_demap_maps)
            PSK_TRY(alloc_zeroed(h->d_demap_maps, psk::kDemapSlots, "demap maps"));
        PSK_TRY(h->dpass.wait());  // (no launch is still reading the slot)
        const psk::DemapMap m = demap_map_make(M, points, labels);
        PSK_HIP(hipMemcpy(h->d_demap_maps + slot, &m, sizeof m, hipMemcpyHostToDevice));
    }
    h->demap_M[slot] = M;  // (a control-plane-only handle checks and counts: M is all it needs)
    return PSK_SOFT_OK;
}

static bool demap_skipped(const psk_soft_demap_in_t &k) { return !k.count || !k.map || !k.soft; }

// what is wrong with a segment that is not skipped, but for its map and its channel; nullptr: nothing
static const char *demap_segment_fault(const psk_soft_demap_in_t &k)
{
    const bool front = (k.flags & PSK_SOFT_DEMAP_FRONT) != 0;
    if (k.flags & ~(uint32_t)(PSK_SOFT_DEMAP_I8 | PSK_SOFT_DEMAP_FRONT))
        return "unknown flag bits";
    if (k.pad)
        return "pad must be zero";
    if ((uintptr_t)k.soft & 7u)
        return "soft must be 8-byte aligned";
    if (!k.out)
        return "out is null";
    if (!(k.flags & PSK_SOFT_DEMAP_I8) && ((uintptr_t)k.out & 3u))
        return "a float32 out must be 4-byte aligned";
    if (k.n_symbols >= psk::kDemapMaxN)
        return "2^30 symbols or more";
    if (k.pos < (front ? -(int64_t)psk::kDemapFront : (int64_t)0))
        return "pos below 0 (below -127 with PSK_SOFT_DEMAP_FRONT)";
    // (no sum of pos and count is formed: pos may be anything up to INT64_MAX; n_symbols < 2^30 and pos >= -127 here)
    if (k.pos > (int64_t)k.n_symbols || (int64_t)k.count > (int64_t)k.n_symbols - k.pos)
        return "pos + count beyond n_symbols";
    if (!psk::dm_finite(k.gain_re) || !psk::dm_finite(k.gain_im) || !psk::dm_finite(k.scale))
        return "a gain or scale that is not finite";
    return nullptr;
}

static psk_soft_status demap_enqueue(psk_soft_handle *h, uint32_t nseg, const psk_soft_demap_in_t *in, hipStream_t stream);

psk_soft_status psk_soft_demap_device(psk_soft_handle_t *h, uint32_t nseg, const psk_soft_demap_in_t *in, void *stream_v)
{
    if (!h || !in || !nseg || nseg > psk::kDemapMaxSegments)
        return fail(PSK_SOFT_ERR_INVALID_ARG, "psk_soft_demap_device: null pointer or a number of segments outside 1 .. 2^20");
    // the refusals, before anything is enqueued or any record changes
    for (uint32_t i = 0; i < nseg; i++) {
        const psk_soft_demap_in_t &k = in[i];
        if (demap_skipped(k))
            continue;
        const char *what = nullptr;
        if (k.map > psk::kDemapSlots || !h->demap_M[k.map - 1u])
            what = "a map slot above 15 or never defined (psk_soft_demap_define)";
        else
            what = demap_segment_fault(k);
        if (!what && (k.flags & PSK_SOFT_DEMAP_FRONT) &&
            (k.channel >= h->nch || h->sync_last.empty() || h->sync_last[k.channel] == psk_soft_handle::kSyncNotSearched))
            what = "PSK_SOFT_DEMAP_FRONT on a channel out of range or one whose last sync call did not search it";
        if (what) {
            char buf[200];
            std::snprintf(buf, sizeof buf, "psk_soft_demap_device: segment %u: %s", i, what);
            return fail(PSK_SOFT_ERR_INVALID_ARG, buf);
        }
    }
    if (h->dry) {
        h->demap.dry.assign(nseg, psk_soft_demap_t{});
        for (uint32_t i = 0; i < nseg; i++) {
            if (demap_skipped(in[i]))
                continue;
            psk_soft_demap_t &r = h->demap.dry[i];
            const uint32_t M = h->demap_M[in[i].map - 1u];
            r.n_symbols = in[i].count;
            r.bits = M == 2u ? 1u : M == 4u ? 2u : 3u;
            r.flags = PSK_SOFT_DEMAP_PLANNED | ((in[i].flags & PSK_SOFT_DEMAP_I8) ? PSK_SOFT_DEMAP_REC_I8 : 0u);
        }
        h->demap_called = true, h->demap_nseg = nseg;
        return PSK_SOFT_OK;
    }
    PSK_HIP(hipSetDevice(h->device));
    hipStream_t stream = stream_v ? (hipStream_t)stream_v : h->stream;
    // (a deferred call's classes end on the side streams: the rows must be complete)
    PSK_HIP(deferred_join(h, stream));
    return demap_enqueue(h, nseg, in, stream);
}

// the fold and the join of a demap call whose arguments have passed
static psk_soft_status demap_enqueue(psk_soft_handle *h, uint32_t nseg, const psk_soft_demap_in_t *in, hipStream_t stream)
{
    // (counted ahead of the descriptors: a call that is refused for its size leaves the last call's records standing)
    PieceCount parts;
    uint32_t ignored;
    for (uint32_t i = 0; i < nseg; i++)
        if (!demap_skipped(in[i]) && !parts.add(psk::demap_pieces(in[i].count), &ignored, &ignored))
            return fail(PSK_SOFT_ERR_LIMIT, "psk_soft_demap_device: too many symbols in one call");
    PSK_TRY(h->demap.grow(h->dpass, nseg));  // (the records are the last call's: nothing of them is kept)
    auto &q = h->dpass.next();
    PSK_TRY(h->dpass.claim(q, nseg, nseg / 4u + 256u));
    parts = PieceCount{};
    for (uint32_t i = 0; i < nseg; i++) {
        psk::DemapDesc &d = q.h_desc[i];
        d = psk::DemapDesc{};
        const psk_soft_demap_in_t &k = in[i];
        if (demap_skipped(k))
            continue;  // (its zero record)
        d.soft = k.soft, d.out = k.out, d.pos = k.pos, d.count = k.count;
        // the history the channel's last sync call read: since that call's flip the slot that is not current
        if (k.pos < 0 && h->sync_last[k.channel] == psk_soft_handle::kSyncSearched)
            d.front = h->sync_hist.out(k.channel);
        d.map = k.map - 1u;
        d.flags = psk::kDemapData | ((k.flags & PSK_SOFT_DEMAP_I8) ? psk::kDemapI8 : 0u);
        (void)parts.add(psk::demap_pieces(k.count), &d.part0, &d.n_piece);  // (counted above: it fits)
        d.gain_re = k.gain_re, d.gain_im = k.gain_im, d.scale = k.scale;
    }
    // (PSK_SOFT_TRACE_LAUNCHES, trace_launch: cnt = segments, tiles = pieces)
    auto mark = [&](const char *what) { return trace_launch(h, what, 0, 0, 0, nseg, parts.total, 0, 0, h->slot, stream); };
    return h->dpass.run(q, nseg, kAllRecords, parts.total, stream, [&]() -> psk_soft_status {
        // the descriptors are up: the records are the new call's from here on, also if a launch below fails
        h->demap_called = true, h->demap_nseg = nseg;
        PSK_HIP(mark("demap_fold"));
        PSK_HIP(psk::launch_demap_fold(q.d_desc, nseg, parts.max_piece, h->d_demap_maps, q.d_part, stream));
        PSK_HIP(mark("demap_join"));
        PSK_HIP(psk::launch_demap_join(q.d_desc, nseg, h->d_demap_maps, q.d_part, h->demap.d, stream));
        return PSK_SOFT_OK;
    });
}

uint64_t psk_soft_demap_bytes(void) { return sizeof(psk_soft_demap_t); }
uint64_t psk_soft_demap_in_bytes(void) { return sizeof(psk_soft_demap_in_t); }
uint32_t psk_soft_demap_piece(void) { return psk::kDemapPiece; }
static_assert(sizeof(psk_soft_demap_t) == 64 && sizeof(psk_soft_demap_in_t) == 64, "include/psk_soft_hip.h states the sizes");

psk_soft_status psk_soft_get_demap(psk_soft_handle_t *h, uint32_t first, uint32_t n, psk_soft_demap_t *rec)
{
    if (!h || !rec || !n || !h->demap_called || (uint64_t)first + n > h->demap_nseg)
        return fail(PSK_SOFT_ERR_INVALID_ARG, "psk_soft_get_demap: null pointer, no psk_soft_demap_device call yet or a range beyond its segments");
    return records_read(h, h->demap, h->dpass, first, n, rec);
}

psk_soft_status psk_soft_demap_host(const float *points, const uint8_t *labels, uint32_t M, const psk_soft_demap_in_t *in, const float *front,
                                    psk_soft_demap_t *rec)
{
    if (!points || !labels || !in || !rec || !demap_map_ok(M, points, labels))
        return fail(PSK_SOFT_ERR_INVALID_ARG, "psk_soft_demap_host: null pointer, an M other than 2, 4, 8, a non-finite point or labels that are not a permutation");
    *rec = psk_soft_demap_t{};
    if (!in->count || !in->soft)
        return PSK_SOFT_OK;
    if (const char *what = demap_segment_fault(*in))
        return fail(PSK_SOFT_ERR_INVALID_ARG, std::string("psk_soft_demap_host: ") + what);
    const psk::DemapMap m = demap_map_make(M, points, labels);
    const bool i8 = (in->flags & PSK_SOFT_DEMAP_I8) != 0;
    const uint32_t B = m.B, T = psk::kDemapThreads, P = psk::kDemapPiece;
    double sum_e = 0.0, sum_err = 0.0;
    for (uint32_t lo = 0; lo < in->count; lo += P) {
        const uint32_t cnt = in->count - lo < P ? in->count - lo : P;
        double le[psk::kDemapThreads] = {}, lr[psk::kDemapThreads] = {};  // the lanes' sums, from 0.0
        for (uint32_t i = 0; i < cnt; i++) {  // (ascending: lane i % 256 meets its symbols in the order t, t + 256, ...)
            const int64_t g = in->pos + (int64_t)lo + (int64_t)i;
            float xr = 0.0f, xi = 0.0f;
            if (g >= 0)
                xr = in->soft[2 * g], xi = in->soft[2 * g + 1];
            else if (front)
                xr = front[2 * (g + (int64_t)psk::kDemapFront)], xi = front[2 * (g + (int64_t)psk::kDemapFront) + 1];
            float e, dmin, v[psk::kDemapMaxB];
            if (psk::dm_symbol(m, xr, xi, in->gain_re, in->gain_im, in->scale, &e, &dmin, v)) {
                le[i % T] += (double)e, lr[i % T] += (double)dmin;
                rec->n_finite++;
            }
            for (uint32_t j = 0; j < B; j++) {
                const uint64_t at = (uint64_t)(lo + i) * B + j;
                rec->n_nan += v[j] != v[j] ? 1u : 0u;
                if (i8) {
                    uint32_t clip = 0;
                    static_cast<int8_t *>(in->out)[at] = (int8_t)psk::dm_i8(v[j], &clip);
                    rec->n_clip += clip;
                } else {
                    static_cast<float *>(in->out)[at] = psk::dm_f32(v[j]);
                }
            }
        }
        // the xor tree across each wave (every lane: s += the s of lane ^ offset), then the waves in order from wave 0's value
        double pe = 0.0, pr = 0.0;
        for (uint32_t w = 0; w < T / 64u; w++) {
            for (uint32_t off = 32; off >= 1; off >>= 1) {
                double ne[64], nr[64];
                for (uint32_t l = 0; l < 64; l++) ne[l] = le[64 * w + l] + le[64 * w + (l ^ off)], nr[l] = lr[64 * w + l] + lr[64 * w + (l ^ off)];
                std::memcpy(le + 64 * w, ne, sizeof ne), std::memcpy(lr + 64 * w, nr, sizeof nr);
            }
            pe = w ? pe + le[64 * w] : le[0];
            pr = w ? pr + lr[64 * w] : lr[0];
        }
        // the pieces in ascending order, from piece 0's
        sum_e = lo ? sum_e + pe : pe;
        sum_err = lo ? sum_err + pr : pr;
    }
    rec->n_symbols = in->count;
    rec->sum_e = sum_e, rec->sum_err = sum_err;
    rec->bits = B;
    rec->flags = PSK_SOFT_DEMAP_DATA | (i8 ? PSK_SOFT_DEMAP_REC_I8 : 0u);
    return PSK_SOFT_OK;
}

psk_soft_status psk_soft_demap_gain(const psk_soft_sync_derived_t *d, uint32_t M, uint32_t flags, float gain[2])
{
    if (!d || !gain || (M != 2u && M != 4u && M != 8u) || (flags & ~(uint32_t)(PSK_SOFT_DEMAP_GAIN_RESIDUAL | PSK_SOFT_DEMAP_GAIN_UNIT)))
        return fail(PSK_SOFT_ERR_INVALID_ARG, "psk_soft_demap_gain: null pointer, an M other than 2, 4, 8 or unknown flags");
    if (d->rotation < 0 || d->rotation >= (int32_t)M || !std::isfinite(d->amplitude) || !(d->amplitude > 0.0) ||
        ((flags & PSK_SOFT_DEMAP_GAIN_RESIDUAL) && !std::isfinite(d->residual)))
        return fail(PSK_SOFT_ERR_INVALID_ARG, "psk_soft_demap_gain: a rotation outside 0 .. M-1, an amplitude that is not finite and positive or a residual that is not finite");
    // cos and sin of k * 2 pi / 8, exactly
    const double s = 0.70710678118654752440;  // M_SQRT1_2
    const double ct[8] = {1.0, s, 0.0, -s, -1.0, -s, 0.0, s}, st[8] = {0.0, s, 1.0, s, 0.0, -s, -1.0, -s};
    const uint32_t k = (uint32_t)d->rotation * (8u / M);
    double c = ct[k], sn = st[k];
    if (flags & PSK_SOFT_DEMAP_GAIN_RESIDUAL) {
        const double cr = std::cos(d->residual), sr = std::sin(d->residual);
        const double c2 = c * cr - sn * sr, s2 = c * sr + sn * cr;
        c = c2, sn = s2;
    }
    // exp(-i theta) / amplitude
    double gr = c, gi = 0.0 - sn;
    if (!(flags & PSK_SOFT_DEMAP_GAIN_UNIT))
        gr /= d->amplitude, gi /= d->amplitude;
    gain[0] = (float)gr, gain[1] = (float)gi;
    return PSK_SOFT_OK;
}

// ---- psk_soft_viterbi_device: frames of int8 LLRs as payload bits (include/psk_soft_hip.h, psk_viterbi.hip) ----
// Behind the demap call: one launch on the caller's stream, one wave per frame, one record per frame of the call; a ring of its
// own like the demapper's, whose "partials" are the decision words of the frames in flight.  Nothing of the control plane, of the
// demodulator's state or of any other record is read or written.
static psk::ViterbiCode viterbi_code_make(uint32_t K, uint32_t n, const uint32_t *g, uint32_t P, uint32_t keep)
{
    psk::ViterbiCode c = {};
    c.K = K, c.n = n, c.P = P, c.keep = keep;
    for (uint32_t j = 0; j < n; j++) c.g[j] = g[j];
    return c;
}

psk_soft_status psk_soft_viterbi_define(psk_soft_handle_t *h, uint32_t slot, uint32_t K, uint32_t n, const uint32_t *g, uint32_t P, uint32_t keep)
{
    if (!h || !g || slot >= psk::kViterbiSlots || !psk::vt_code_ok(K, n, g, P, keep))
        return fail(PSK_SOFT_ERR_INVALID_ARG, "psk_soft_viterbi_define: null pointer, a slot above 15, K outside 3 .. 7, n outside 2 .. 4, a polynomial that is 0 or has bits at or above K, polynomials that tap neither bit K-1 nor bit 0, P outside 1 .. 16, n P above 32 or a keep that is 0 or has bits at or above n P");
    const psk::ViterbiCode c = viterbi_code_make(K, n, g, P, keep);
    if (!h->dry) {
        PSK_HIP(hipSetDevice(h->device));
        if (!h->d_viterbi_codes)
            PSK_TRY(alloc_zeroed(h->d_viterbi_codes, psk::kViterbiSlots, "viterbi codes"));
        PSK_TRY(h->vpass.wait());  // (no launch is still reading the slot)
        PSK_HIP(hipMemcpy(h->d_viterbi_codes + slot, &c, sizeof c, hipMemcpyHostToDevice));
    }
    h->viterbi_code[slot] = c;
    return PSK_SOFT_OK;
}

static bool viterbi_skipped(const psk_soft_viterbi_in_t &k) { return !k.n_steps || !k.code || !k.llr; }

// what is wrong with a frame that is not skipped, given the K of its code; nullptr: nothing
static const char *viterbi_frame_fault(const psk_soft_viterbi_in_t &k, uint32_t K)
{
    if (k.flags & ~psk::kViterbiFlagMask)
        return "unknown flag bits";
    if (k.pad)
        return "pad must be zero";
    if (!k.out)
        return "out is null";
    if (k.n_steps > psk::kViterbiMaxSteps)
        return "more than 65536 steps";
    if ((k.flags & PSK_SOFT_VITERBI_TERMINATED) && k.n_steps < K - 1u)
        return "PSK_SOFT_VITERBI_TERMINATED with fewer than K-1 steps";
    return nullptr;
}

psk_soft_status psk_soft_viterbi_device(psk_soft_handle_t *h, uint32_t nframe, const psk_soft_viterbi_in_t *in, void *stream_v)
{
    if (!h || !in || !nframe || nframe > psk::kViterbiMaxFrames)
        return fail(PSK_SOFT_ERR_INVALID_ARG, "psk_soft_viterbi_device: null pointer or a number of frames outside 1 .. 2^20");
    // the refusals, before anything is enqueued or any record changes
    uint32_t max_steps = 0;
    for (uint32_t i = 0; i < nframe; i++) {
        const psk_soft_viterbi_in_t &k = in[i];
        if (viterbi_skipped(k))
            continue;
        const char *what = nullptr;
        if (k.code > psk::kViterbiSlots || !h->viterbi_code[k.code - 1u].K)
            what = "a code slot above 15 or never defined (psk_soft_viterbi_define)";
        else
            what = viterbi_frame_fault(k, h->viterbi_code[k.code - 1u].K);
        if (what) {
            char buf[200];
            std::snprintf(buf, sizeof buf, "psk_soft_viterbi_device: frame %u: %s", i, what);
            return fail(PSK_SOFT_ERR_INVALID_ARG, buf);
        }
        max_steps = k.n_steps > max_steps ? k.n_steps : max_steps;
    }
    auto n_llr_of = [&](const psk_soft_viterbi_in_t &k) {
        const psk::ViterbiCode &c = h->viterbi_code[k.code - 1u];
        return (uint32_t)psk::vt_count(c.n, c.P, c.keep, k.n_steps);
    };
    if (h->dry) {
        h->viterbi.dry.assign(nframe, psk_soft_viterbi_t{});
        for (uint32_t i = 0; i < nframe; i++) {
            if (viterbi_skipped(in[i]))
                continue;
            psk_soft_viterbi_t &r = h->viterbi.dry[i];
            r.n_steps = in[i].n_steps;
            r.n_llr = n_llr_of(in[i]);
            r.n_bits = psk::viterbi_bits(h->viterbi_code[in[i].code - 1u].K, in[i].n_steps, in[i].flags);
            r.flags = PSK_SOFT_VITERBI_PLANNED | (in[i].flags << 1);
        }
        h->viterbi_called = true, h->viterbi_nframe = nframe;
        return PSK_SOFT_OK;
    }
    PSK_HIP(hipSetDevice(h->device));
    hipStream_t stream = stream_v ? (hipStream_t)stream_v : h->stream;
    // (a deferred call's classes end on the side streams: whatever made the LLRs must be complete)
    PSK_HIP(deferred_join(h, stream));
    // the frames in flight: one per workgroup, each with room for the longest frame's decisions, within the scratch bound
    const uint32_t steps_cap = max_steps ? (max_steps + psk::kViterbiChunk - 1u) / psk::kViterbiChunk * psk::kViterbiChunk : psk::kViterbiChunk;
    uint64_t grid = psk::kViterbiScratchWords / steps_cap;  // (steps_cap <= 65536: at least 512)
    grid = grid < nframe ? grid : nframe;
    grid = grid < 65535u ? grid : 65535u;
    PSK_TRY(h->viterbi.grow(h->vpass, nframe));  // (the records are the last call's: nothing of them is kept)
    auto &q = h->vpass.next();
    PSK_TRY(h->vpass.claim(q, nframe, nframe / 4u + 256u));
    for (uint32_t i = 0; i < nframe; i++) {
        psk::ViterbiDesc &d = q.h_desc[i];
        d = psk::ViterbiDesc{};
        const psk_soft_viterbi_in_t &k = in[i];
        if (viterbi_skipped(k))
            continue;  // (its zero record)
        d.llr = k.llr, d.out = k.out, d.n_steps = k.n_steps, d.code = k.code - 1u;
        d.flags = psk::kViterbiData | (k.flags << 1);
        d.n_llr = n_llr_of(k);
    }
    // (PSK_SOFT_TRACE_LAUNCHES, trace_launch: cnt = frames, tiles = workgroups)
    return h->vpass.run(q, nframe, kAllRecords, grid * steps_cap, stream, [&]() -> psk_soft_status {
        // the descriptors are up: the records are the new call's from here on, also if the launch below fails
        h->viterbi_called = true, h->viterbi_nframe = nframe;
        PSK_HIP(trace_launch(h, "viterbi", 0, 0, 0, nframe, grid, 0, 0, h->slot, stream));
        PSK_HIP(psk::launch_viterbi(q.d_desc, nframe, (uint32_t)grid, steps_cap, h->d_viterbi_codes, q.d_part, h->viterbi.d, stream));
        return PSK_SOFT_OK;
    });
}

uint64_t psk_soft_viterbi_bytes(void) { return sizeof(psk_soft_viterbi_t); }
uint64_t psk_soft_viterbi_in_bytes(void) { return sizeof(psk_soft_viterbi_in_t); }
static_assert(sizeof(psk_soft_viterbi_t) == 64 && sizeof(psk_soft_viterbi_in_t) == 32, "include/psk_soft_hip.h states the sizes");
static_assert(PSK_SOFT_VITERBI_DATA == psk::kViterbiData && PSK_SOFT_VITERBI_REC_PACKED == PSK_SOFT_VITERBI_PACKED << 1 &&
                  PSK_SOFT_VITERBI_REC_TERMINATED == PSK_SOFT_VITERBI_TERMINATED << 1 &&
                  PSK_SOFT_VITERBI_REC_ANY_START == PSK_SOFT_VITERBI_ANY_START << 1,
              "the record's flags are the frame's shifted left by one");

psk_soft_status psk_soft_get_viterbi(psk_soft_handle_t *h, uint32_t first, uint32_t n, psk_soft_viterbi_t *rec)
{
    if (!h || !rec || !n || !h->viterbi_called || (uint64_t)first + n > h->viterbi_nframe)
        return fail(PSK_SOFT_ERR_INVALID_ARG, "psk_soft_get_viterbi: null pointer, no psk_soft_viterbi_device call yet or a range beyond its frames");
    return records_read(h, h->viterbi, h->vpass, first, n, rec);
}

uint64_t psk_soft_viterbi_count(uint32_t K, uint32_t n, uint32_t P, uint32_t keep, uint64_t n_steps)
{
    (void)K;
    if (n < 2u || n > psk::kViterbiMaxN || !P || P > psk::kViterbiMaxP || n * P > 32u || !keep || (n * P < 32u && (keep >> (n * P))))
        return 0;
    return (n_steps / P) * psk::vt_popc(keep) + psk::vt_count(n, P, keep, (uint32_t)(n_steps % P));
}

psk_soft_status psk_soft_viterbi_encode_host(uint32_t K, uint32_t n, const uint32_t *g, uint32_t P, uint32_t keep, const uint8_t *bits,
                                             uint32_t n_steps, uint8_t *code_bits_out)
{
    if (!g || !psk::vt_code_ok(K, n, g, P, keep) || (n_steps && (!bits || !code_bits_out)))
        return fail(PSK_SOFT_ERR_INVALID_ARG, "psk_soft_viterbi_encode_host: null pointer or a code psk_soft_viterbi_define refuses");
    const psk::ViterbiCode c = viterbi_code_make(K, n, g, P, keep);
    uint32_t s = 0, phase = 0;
    for (uint32_t t = 0; t < n_steps; t++) {
        const uint32_t r = ((uint32_t)(bits[t] & 1u) << (K - 1u)) | s;
        const uint32_t cb = psk::vt_code_bits(c, r), km = psk::vt_keep_of(n, keep, phase);
        phase = psk::vt_next_phase(P, phase);
        for (uint32_t j = 0; j < n; j++)
            if ((km >> j) & 1u)
                *code_bits_out++ = (uint8_t)((cb >> j) & 1u);
        s = r >> 1;
    }
    return PSK_SOFT_OK;
}

psk_soft_status psk_soft_viterbi_host(uint32_t K, uint32_t n, const uint32_t *g, uint32_t P, uint32_t keep, const psk_soft_viterbi_in_t *in,
                                      psk_soft_viterbi_t *rec)
{
    if (!g || !in || !rec || !psk::vt_code_ok(K, n, g, P, keep))
        return fail(PSK_SOFT_ERR_INVALID_ARG, "psk_soft_viterbi_host: null pointer or a code psk_soft_viterbi_define refuses");
    *rec = psk_soft_viterbi_t{};
    if (viterbi_skipped(*in))
        return PSK_SOFT_OK;
    if (const char *what = viterbi_frame_fault(*in, K))
        return fail(PSK_SOFT_ERR_INVALID_ARG, std::string("psk_soft_viterbi_host: ") + what);
    const psk::ViterbiCode c = viterbi_code_make(K, n, g, P, keep);
    const uint32_t T = in->n_steps, NS = 1u << (K - 1u), mask = NS - 1u;
    uint32_t bits0[64], bits1[64];
    int32_t pm[64], nw[64];
    for (uint32_t s = 0; s < NS; s++) {
        bits0[s] = psk::vt_branch_bits(c, s, 0u), bits1[s] = psk::vt_branch_bits(c, s, 1u);
        pm[s] = ((in->flags & PSK_SOFT_VITERBI_ANY_START) || s == 0u) ? 0 : psk::kViterbiUnreached;
    }
    // forward: the decisions of a step are one word, bit s the decision of state s
    std::vector<uint64_t> dec(T);
    const int8_t *q = in->llr;
    uint32_t phase = 0;
    for (uint32_t t = 0; t < T; t++) {
        const uint32_t km = psk::vt_keep_of(n, keep, phase);
        phase = psk::vt_next_phase(P, phase);
        int32_t l[psk::kViterbiMaxN] = {};
        for (uint32_t j = 0; j < n; j++)
            if ((km >> j) & 1u)
                l[j] = *q++;
        uint64_t w = 0;
        for (uint32_t s = 0; s < NS; s++) {
            const uint32_t p0 = (s << 1) & mask;
            uint32_t d;
            nw[s] = psk::vt_acs(pm[p0], psk::vt_bm<psk::kViterbiMaxN>(bits0[s], l), pm[p0 | 1u], psk::vt_bm<psk::kViterbiMaxN>(bits1[s], l), &d);
            w |= (uint64_t)d << s;
        }
        for (uint32_t s = 0; s < NS; s++) pm[s] = nw[s];
        dec[t] = w;
    }
    const uint64_t n_llr = (uint64_t)(q - in->llr);
    // the end state: 0, or the first maximum
    uint32_t s = 0;
    if (!(in->flags & PSK_SOFT_VITERBI_TERMINATED))
        for (uint32_t k = 1; k < NS; k++)
            if (pm[k] > pm[s])
                s = k;
    rec->end_state = s, rec->metric = pm[s];
    // traceback; the path's code bits against the LLRs, walked from the back
    const uint32_t n_bits = psk::viterbi_bits(K, T, in->flags);
    const bool packed = (in->flags & PSK_SOFT_VITERBI_PACKED) != 0;
    uint8_t *const out = (uint8_t *)in->out;
    if (packed)
        std::memset(out, 0, (n_bits + 7u) / 8u);
    uint32_t sum_abs = 0, n_flip = 0, n_zero = 0;
    for (uint32_t t = T; t-- > 0u;) {
        const uint32_t u = s >> (K - 2u);
        const uint32_t prev = ((s << 1) & mask) | (uint32_t)((dec[t] >> s) & 1u);
        const uint32_t cb = psk::vt_code_bits(c, (u << (K - 1u)) | prev), km = psk::vt_keep_of(n, keep, t % P);
        const int8_t *const lt = in->llr + psk::vt_count(n, P, keep, t);
        for (uint32_t j = 0, k = 0; j < n; j++)
            if ((km >> j) & 1u)
                psk::vt_tally((int32_t)lt[k++], (cb >> j) & 1u, &sum_abs, &n_flip, &n_zero);
        if (t < n_bits) {
            if (packed)
                out[t >> 3] |= (uint8_t)(u << (7u - (t & 7u)));
            else
                out[t] = (uint8_t)u;
        }
        s = prev;
    }
    rec->n_steps = T, rec->n_llr = n_llr;
    rec->sum_abs = sum_abs, rec->n_flip = n_flip, rec->n_zero = n_zero;
    rec->start_state = s, rec->n_bits = n_bits;
    rec->flags = PSK_SOFT_VITERBI_DATA | (in->flags << 1);
    return PSK_SOFT_OK;
}

// ---- psk_soft_rs_device: frames of bytes as corrected bytes (include/psk_soft_rs.h, psk_rs.hip) ----
// Behind the viterbi call: one launch on the caller's stream, one wave per frame, one record per frame of the call; a ring of its
// own like the decoder's, without partials.  Nothing of the control plane, of the demodulator's state or of any other record is
// read or written.
static psk::RsCode rs_code_make(uint32_t gfpoly, uint32_t fcr, uint32_t prim, uint32_t nroots, uint32_t n, uint32_t depth, uint32_t mask_len)
{
    psk::RsCode c = {};
    c.gfpoly = gfpoly, c.fcr = fcr, c.prim = prim, c.nroots = nroots, c.n = n, c.depth = depth, c.mask_len = mask_len;
    return c;
}

static const char *const kRsCodeFault =
    "null pointer, a slot above 15, gfpoly outside 0x100 .. 0x1ff or not primitive, fcr above 254, prim outside 1 .. 254 or not coprime to "
    "255, nroots outside 2 .. 64, n outside nroots + 1 .. 255, depth outside 1 .. 8, mask_len above n depth or a null mask with mask_len > 0";

psk_soft_status psk_soft_rs_define(psk_soft_handle_t *h, uint32_t slot, uint32_t gfpoly, uint32_t fcr, uint32_t prim, uint32_t nroots, uint32_t n,
                                   uint32_t depth, const uint8_t *mask, uint32_t mask_len)
{
    if (!h || slot >= psk::kRsSlots || !psk::rs_code_ok(gfpoly, fcr, prim, nroots, n, depth, mask_len) || (mask_len && !mask))
        return fail(PSK_SOFT_ERR_INVALID_ARG, std::string("psk_soft_rs_define: ") + kRsCodeFault);
    const psk::RsCode c = rs_code_make(gfpoly, fcr, prim, nroots, n, depth, mask_len);
    if (!h->dry) {
        PSK_HIP(hipSetDevice(h->device));
        if (!h->d_rs_codes)
            PSK_TRY(alloc_zeroed(h->d_rs_codes, psk::kRsSlots, "rs codes"));
        if (!h->d_rs_masks)
            PSK_TRY(alloc_zeroed(h->d_rs_masks, (size_t)psk::kRsSlots * psk::kRsMaskStride, "rs masks"));
        PSK_TRY(h->rpass.wait());  // (no launch is still reading the slot)
        if (mask_len)
            PSK_HIP(hipMemcpy(h->d_rs_masks + (size_t)slot * psk::kRsMaskStride, mask, mask_len, hipMemcpyHostToDevice));
        PSK_HIP(hipMemcpy(h->d_rs_codes + slot, &c, sizeof c, hipMemcpyHostToDevice));
    }
    h->rs_code[slot] = c;
    return PSK_SOFT_OK;
}

static bool rs_skipped(const psk_soft_rs_in_t &k) { return !k.code || !k.in; }

// what is wrong with a frame that is not skipped; nullptr: nothing
static const char *rs_frame_fault(const psk_soft_rs_in_t &k)
{
    if (k.flags & ~psk::kRsFlagMask)
        return "unknown flag bits";
    if (k.pad[0] || k.pad[1])
        return "pad must be zero";
    if (!k.out)
        return "out is null";
    return nullptr;
}

psk_soft_status psk_soft_rs_device(psk_soft_handle_t *h, uint32_t nframe, const psk_soft_rs_in_t *in, void *stream_v)
{
    if (!h || !in || !nframe || nframe > psk::kRsMaxFrames)
        return fail(PSK_SOFT_ERR_INVALID_ARG, "psk_soft_rs_device: null pointer or a number of frames outside 1 .. 2^20");
    // the refusals, before anything is enqueued or any record changes
    for (uint32_t i = 0; i < nframe; i++) {
        const psk_soft_rs_in_t &k = in[i];
        if (rs_skipped(k))
            continue;
        const char *what = nullptr;
        if (k.code > psk::kRsSlots || !h->rs_code[k.code - 1u].gfpoly)
            what = "a code slot above 15 or never defined (psk_soft_rs_define)";
        else
            what = rs_frame_fault(k);
        if (what) {
            char buf[200];
            std::snprintf(buf, sizeof buf, "psk_soft_rs_device: frame %u: %s", i, what);
            return fail(PSK_SOFT_ERR_INVALID_ARG, buf);
        }
    }
    if (h->dry) {
        h->rs.dry.assign(nframe, psk_soft_rs_t{});
        for (uint32_t i = 0; i < nframe; i++) {
            if (rs_skipped(in[i]))
                continue;
            const psk::RsCode &c = h->rs_code[in[i].code - 1u];
            psk_soft_rs_t &r = h->rs.dry[i];
            r.n = (uint16_t)c.n, r.k = (uint16_t)(c.n - c.nroots), r.depth = (uint8_t)c.depth, r.nroots = (uint8_t)c.nroots;
            r.flags = PSK_SOFT_RS_PLANNED | (in[i].flags << 1);
        }
        h->rs_called = true, h->rs_nframe = nframe;
        return PSK_SOFT_OK;
    }
    PSK_HIP(hipSetDevice(h->device));
    hipStream_t stream = stream_v ? (hipStream_t)stream_v : h->stream;
    // (a deferred call's classes end on the side streams: whatever made the bytes must be complete)
    PSK_HIP(deferred_join(h, stream));
    const uint32_t grid = nframe < psk::kRsMaxGrid ? nframe : psk::kRsMaxGrid;
    PSK_TRY(h->rs.grow(h->rpass, nframe));  // (the records are the last call's: nothing of them is kept)
    auto &q = h->rpass.next();
    PSK_TRY(h->rpass.claim(q, nframe, nframe / 4u + 256u));
    for (uint32_t i = 0; i < nframe; i++) {
        psk::RsDesc &d = q.h_desc[i];
        d = psk::RsDesc{};
        const psk_soft_rs_in_t &k = in[i];
        if (rs_skipped(k))
            continue;  // (its zero record)
        d.in = k.in, d.out = k.out, d.code = k.code - 1u;
        d.flags = psk::kRsData | (k.flags << 1);
    }
    // (PSK_SOFT_TRACE_LAUNCHES, trace_launch: cnt = frames, tiles = workgroups)
    return h->rpass.run(q, nframe, kAllRecords, 0, stream, [&]() -> psk_soft_status {
        // the descriptors are up: the records are the new call's from here on, also if the launch below fails
        h->rs_called = true, h->rs_nframe = nframe;
        PSK_HIP(trace_launch(h, "rs", 0, 0, 0, nframe, grid, 0, 0, h->slot, stream));
        PSK_HIP(psk::launch_rs(q.d_desc, nframe, grid, h->d_rs_codes, h->d_rs_masks, h->rs.d, stream));
        return PSK_SOFT_OK;
    });
}

uint64_t psk_soft_rs_bytes(void) { return sizeof(psk_soft_rs_t); }
uint64_t psk_soft_rs_in_bytes(void) { return sizeof(psk_soft_rs_in_t); }
static_assert(sizeof(psk_soft_rs_t) == 64 && sizeof(psk_soft_rs_in_t) == 32, "include/psk_soft_rs.h states the sizes");
static_assert(offsetof(psk_soft_rs_t, n_err) == 16 && offsetof(psk_soft_rs_t, n_bit) == 24 && offsetof(psk_soft_rs_t, depth) == 8,
              "psk_rs.hip stores the record as eight words");
static_assert(PSK_SOFT_RS_DATA == psk::kRsData && PSK_SOFT_RS_REC_WITH_PARITY == PSK_SOFT_RS_WITH_PARITY << 1,
              "the record's flags are the frame's shifted left by one");

psk_soft_status psk_soft_get_rs(psk_soft_handle_t *h, uint32_t first, uint32_t n, psk_soft_rs_t *rec)
{
    if (!h || !rec || !n || !h->rs_called || (uint64_t)first + n > h->rs_nframe)
        return fail(PSK_SOFT_ERR_INVALID_ARG, "psk_soft_get_rs: null pointer, no psk_soft_rs_device call yet or a range beyond its frames");
    return records_read(h, h->rs, h->rpass, first, n, rec);
}

// the generator g(x) = prod (x - root m), g[d] the coefficient of x^d, d = 0 .. nroots
static void rs_generator(const psk::RsCode &c, uint8_t *g)
{
    g[0] = 1;
    for (uint32_t m = 0; m < c.nroots; m++) {
        const uint32_t root = psk::rs_root(c, m);
        g[m + 1u] = 0;
        for (uint32_t d = m + 1u; d > 0u; d--) g[d] = (uint8_t)(g[d - 1u] ^ psk::gf_mul(c.gfpoly, g[d], root));
        g[0] = (uint8_t)psk::gf_mul(c.gfpoly, g[0], root);
    }
}

psk_soft_status psk_soft_rs_encode_host(uint32_t gfpoly, uint32_t fcr, uint32_t prim, uint32_t nroots, uint32_t n, uint32_t depth,
                                        const uint8_t *mask, uint32_t mask_len, const uint8_t *data, uint8_t *frame_out)
{
    if (!data || !frame_out || !psk::rs_code_ok(gfpoly, fcr, prim, nroots, n, depth, mask_len) || (mask_len && !mask))
        return fail(PSK_SOFT_ERR_INVALID_ARG, std::string("psk_soft_rs_encode_host: ") + kRsCodeFault);
    const psk::RsCode c = rs_code_make(gfpoly, fcr, prim, nroots, n, depth, mask_len);
    const uint32_t k = n - nroots;
    uint8_t g[psk::kRsMaxRoots + 1u];
    rs_generator(c, g);
    for (uint32_t j = 0; j < depth; j++) {
        uint8_t par[psk::kRsMaxRoots] = {};  // par[d]: the coefficient of x^d of the remainder so far
        for (uint32_t i = 0; i < k; i++) {
            const uint8_t b = data[i * depth + j];
            frame_out[i * depth + j] = b;
            const uint32_t fb = b ^ par[nroots - 1u];
            for (uint32_t d = nroots - 1u; d > 0u; d--) par[d] = (uint8_t)(par[d - 1u] ^ psk::gf_mul(gfpoly, fb, g[d]));
            par[0] = (uint8_t)psk::gf_mul(gfpoly, fb, g[0]);
        }
        for (uint32_t i = 0; i < nroots; i++) frame_out[(k + i) * depth + j] = par[nroots - 1u - i];
    }
    for (uint32_t q = 0; q < mask_len; q++) frame_out[q] ^= mask[q];
    return PSK_SOFT_OK;
}

// One received word w[0 .. n-1] corrected in place, the definition on the host: syndromes, Berlekamp-Massey, a search of the n
// positions, Forney, and the outcome held to the definition.  Returns the number of bytes changed, or kRsFailed with w unchanged.
static uint32_t rs_decode_word(const psk::RsCode &c, uint8_t *w, uint32_t *n_bit)
{
    const uint32_t gp = c.gfpoly, nroots = c.nroots, n = c.n, t = nroots / 2u;
    *n_bit = 0;
    uint8_t S[psk::kRsMaxRoots], root[psk::kRsMaxRoots];
    uint32_t any = 0;
    for (uint32_t m = 0; m < nroots; m++) {
        root[m] = (uint8_t)psk::rs_root(c, m);
        uint32_t s = 0;
        for (uint32_t i = 0; i < n; i++) s = psk::gf_mul(gp, s, root[m]) ^ w[i];
        S[m] = (uint8_t)s, any |= s;
    }
    if (!any)
        return 0;
    uint8_t lam[psk::kRsMaxRoots + 2u] = {1}, B[psk::kRsMaxRoots + 2u] = {1}, T[psk::kRsMaxRoots + 2u];
    uint32_t len = 0;
    for (uint32_t r = 0; r < nroots; r++) {
        uint32_t delta = 0;
        for (uint32_t i = 0; i <= r; i++) delta ^= psk::gf_mul(gp, lam[i], S[r - i]);
        for (uint32_t d = nroots + 1u; d > 0u; d--) B[d] = B[d - 1u];  // x B
        B[0] = 0;
        if (!delta)
            continue;
        for (uint32_t d = 0; d <= nroots + 1u; d++) T[d] = (uint8_t)(lam[d] ^ psk::gf_mul(gp, delta, B[d]));
        if (2u * len <= r) {
            const uint32_t inv = psk::gf_inv(gp, delta);
            for (uint32_t d = 0; d <= nroots + 1u; d++) B[d] = (uint8_t)psk::gf_mul(gp, lam[d], inv);
            len = r + 1u - len;
        }
        std::memcpy(lam, T, sizeof T);
    }
    uint32_t deg = 0;
    for (uint32_t d = 0; d <= nroots + 1u; d++)
        if (lam[d])
            deg = d;
    if (len > t || deg != len)
        return psk::kRsFailed;
    uint8_t om[psk::kRsMaxRoots] = {};
    for (uint32_t L = 0; L < deg; L++)
        for (uint32_t i = 0; i <= L; i++) om[L] ^= (uint8_t)psk::gf_mul(gp, lam[i], S[L - i]);
    uint8_t e[255] = {};
    uint32_t nroot = 0;
    for (uint32_t i = 0; i < n; i++) {
        const uint32_t p = n - 1u - i, xinv = psk::rs_locator_inv(c, p);
        uint32_t lamv = 0, omv = 0, der = 0, xp = 1u, xprev = 0u;
        for (uint32_t d = 0; d <= deg; d++) {
            lamv ^= psk::gf_mul(gp, lam[d], xp);
            omv ^= d < deg ? psk::gf_mul(gp, om[d], xp) : 0u;
            der ^= (d & 1u) ? psk::gf_mul(gp, lam[d], xprev) : 0u;
            xprev = xp;
            xp = psk::gf_mul(gp, xp, xinv);
        }
        if (lamv)
            continue;
        nroot++;
        const uint32_t v = der ? psk::rs_magnitude(c, p, omv, der) : 0u;
        if (!v)
            return psk::kRsFailed;
        e[i] = (uint8_t)v;
    }
    if (nroot != deg)
        return psk::kRsFailed;
    for (uint32_t m = 0; m < nroots; m++) {  // the pattern's syndromes are the word's
        uint32_t s = 0;
        for (uint32_t i = 0; i < n; i++) s = psk::gf_mul(gp, s, root[m]) ^ e[i];
        if (s != S[m])
            return psk::kRsFailed;
    }
    for (uint32_t i = 0; i < n; i++) {
        w[i] ^= e[i];
        *n_bit += (uint32_t)__builtin_popcount(e[i]);
    }
    return deg;
}

psk_soft_status psk_soft_rs_host(uint32_t gfpoly, uint32_t fcr, uint32_t prim, uint32_t nroots, uint32_t n, uint32_t depth, const uint8_t *mask,
                                 uint32_t mask_len, const psk_soft_rs_in_t *in, psk_soft_rs_t *rec)
{
    if (!in || !rec || !psk::rs_code_ok(gfpoly, fcr, prim, nroots, n, depth, mask_len) || (mask_len && !mask))
        return fail(PSK_SOFT_ERR_INVALID_ARG, std::string("psk_soft_rs_host: ") + kRsCodeFault);
    *rec = psk_soft_rs_t{};
    if (rs_skipped(*in))
        return PSK_SOFT_OK;
    if (const char *what = rs_frame_fault(*in))
        return fail(PSK_SOFT_ERR_INVALID_ARG, std::string("psk_soft_rs_host: ") + what);
    const psk::RsCode c = rs_code_make(gfpoly, fcr, prim, nroots, n, depth, mask_len);
    const uint32_t k = n - nroots, n_out = (in->flags & PSK_SOFT_RS_WITH_PARITY) ? n : k;
    for (uint32_t j = 0; j < depth; j++) {
        uint8_t w[255];
        for (uint32_t i = 0; i < n; i++) {
            const uint32_t off = i * depth + j;
            w[i] = (uint8_t)(in->in[off] ^ (off < mask_len ? mask[off] : 0u));
        }
        uint32_t n_bit = 0;
        rec->n_err[j] = (uint8_t)rs_decode_word(c, w, &n_bit);
        rec->n_bit[j] = (uint16_t)n_bit;
        for (uint32_t i = 0; i < n_out; i++) in->out[i * depth + j] = w[i];
    }
    rec->n = (uint16_t)n, rec->k = (uint16_t)k, rec->depth = (uint8_t)depth, rec->nroots = (uint8_t)nroots;
    rec->flags = PSK_SOFT_RS_DATA | (in->flags << 1);
    return PSK_SOFT_OK;
}

// ---- psk_soft_frame_search_device, psk_soft_frame_cut_device: frames as aligned bytes (include/psk_soft_frame.h, psk_frame.hip) ----
// Between the viterbi call and the rs call, on the caller's stream.  The search is a pass of the reduction-pass layer with
// partials (a fold over tiles of phases or windows, a join per stream); the cut is one launch with a ring of its own like the rs
// entry's.  Nothing of the control plane, of the demodulator's state or of any other record is read or written.
static const char *const kFrameWordFault = "null pointer, a slot above 15, length outside 1 .. 64, bits of word or care at length and above, or care == 0";
static const char *const kFrameFormatFault =
    "null pointer, a slot above 15, branches outside 1 .. 255, cell above 255 or branches (branches - 1) cell above 2^24";

psk_soft_status psk_soft_frame_word_define(psk_soft_handle_t *h, uint32_t slot, uint32_t length, uint64_t word, uint64_t care)
{
    if (!h || slot >= psk::kFrameSlots || !psk::frame_word_ok(length, word, care))
        return fail(PSK_SOFT_ERR_INVALID_ARG, std::string("psk_soft_frame_word_define: ") + kFrameWordFault);
    if (!h->dry)
        PSK_TRY(h->fpass.wait());  // (the handle's last search launch is behind us)
    h->frame_word[slot] = psk::FrameWord{word, care, length, psk::frame_popcount(care)};
    return PSK_SOFT_OK;
}

static bool frame_search_skipped(const psk_soft_frame_search_in_t &k) { return !k.word || !k.bits; }

// what is wrong with a stream that is not skipped, searched for a word of `ncare` care bits; nullptr: nothing
static const char *frame_search_fault(const psk_soft_frame_search_in_t &k, uint32_t ncare)
{
    if (2ull * k.max_diff >= ncare)
        return "2 max_diff must be below the number of care bits";
    if (k.period > psk::kFrameMaxPeriod)
        return "a period above 2^20";
    if (k.n_bits < 1u || k.n_bits > psk::kFrameMaxBits)
        return "n_bits outside 1 .. 2^31";
    if (k.flags)
        return "unknown flag bits";
    if (k.pad[0] || k.pad[1] || k.pad[2])
        return "pad must be zero";
    return nullptr;
}

static uint32_t frame_windows(uint32_t n_bits, uint32_t length) { return n_bits >= length ? n_bits - length + 1u : 0u; }

psk_soft_status psk_soft_frame_search_device(psk_soft_handle_t *h, uint32_t nstream, const psk_soft_frame_search_in_t *in, void *stream_v)
{
    if (!h || !in || !nstream || nstream > psk::kFrameMaxStreams)
        return fail(PSK_SOFT_ERR_INVALID_ARG, "psk_soft_frame_search_device: null pointer or a number of streams outside 1 .. 2^20");
    // the refusals, before anything is enqueued or any record changes
    PieceCount parts;
    for (uint32_t i = 0; i < nstream; i++) {
        const psk_soft_frame_search_in_t &k = in[i];
        if (frame_search_skipped(k))
            continue;
        const char *what = nullptr;
        if (k.word > psk::kFrameSlots || !h->frame_word[k.word - 1u].length)
            what = "a word slot above 15 or never defined (psk_soft_frame_word_define)";
        else
            what = frame_search_fault(k, h->frame_word[k.word - 1u].ncare);
        uint32_t part0, n_tile;
        if (!what && !parts.add(psk::frame_tiles(frame_windows(k.n_bits, h->frame_word[k.word - 1u].length), k.period), &part0, &n_tile))
            what = "the call would have 2^31 tiles or more";
        if (what) {
            char buf[200];
            std::snprintf(buf, sizeof buf, "psk_soft_frame_search_device: stream %u: %s", i, what);
            return fail(PSK_SOFT_ERR_INVALID_ARG, buf);
        }
    }
    if (h->dry) {
        h->fsearch.dry.assign(nstream, psk_soft_frame_search_t{});
        for (uint32_t i = 0; i < nstream; i++) {
            if (frame_search_skipped(in[i]))
                continue;
            const psk::FrameWord &w = h->frame_word[in[i].word - 1u];
            psk_soft_frame_search_t &r = h->fsearch.dry[i];
            r.flags = PSK_SOFT_FRAME_PLANNED, r.length = w.length, r.n_windows = frame_windows(in[i].n_bits, w.length);
        }
        h->fsearch_called = true, h->fsearch_n = nstream;
        return PSK_SOFT_OK;
    }
    PSK_HIP(hipSetDevice(h->device));
    hipStream_t stream = stream_v ? (hipStream_t)stream_v : h->stream;
    // (a deferred call's classes end on the side streams: whatever made the bits must be complete)
    PSK_HIP(deferred_join(h, stream));
    PSK_TRY(h->fsearch.grow(h->fpass, nstream));  // (the records are the last call's: nothing of them is kept)
    auto &q = h->fpass.next();
    PSK_TRY(h->fpass.claim(q, nstream, nstream / 4u + 256u));
    parts = PieceCount{};
    for (uint32_t i = 0; i < nstream; i++) {
        psk::FrameSearchDesc &d = q.h_desc[i];
        d = psk::FrameSearchDesc{};
        d.part0 = (uint32_t)parts.total;  // (a stream without tiles shares its first partial with the next: the fold's search)
        const psk_soft_frame_search_in_t &k = in[i];
        if (frame_search_skipped(k))
            continue;  // (its zero record)
        const psk::FrameWord &w = h->frame_word[k.word - 1u];
        // whole bytes of bit0 go into the pointer: the kernels count bits in 32
        d.bits = k.bits + (k.bit0 >> 3), d.bit0 = k.bit0 & 7u;
        d.word = w.word, d.care = w.care, d.length = w.length, d.ncare = w.ncare;
        d.n_windows = frame_windows(k.n_bits, w.length), d.max_diff = k.max_diff, d.period = k.period;
        d.flags = psk::kFrameData;
        (void)parts.add(psk::frame_tiles(d.n_windows, d.period), &d.part0, &d.n_tile);
    }
    // (PSK_SOFT_TRACE_LAUNCHES, trace_launch: cnt = streams, tiles = workgroups of the fold)
    return h->fpass.run(q, nstream, kAllRecords, parts.total, stream, [&]() -> psk_soft_status {
        // the descriptors are up: the records are the new call's from here on, also if a launch below fails
        h->fsearch_called = true, h->fsearch_n = nstream;
        PSK_HIP(trace_launch(h, "frame_search", 0, 0, 0, nstream, parts.total, 0, 0, h->slot, stream));
        PSK_HIP(psk::launch_frame_search(q.d_desc, nstream, (uint32_t)parts.total, q.d_part, h->fsearch.d, stream));
        return PSK_SOFT_OK;
    });
}

psk_soft_status psk_soft_get_frame_search(psk_soft_handle_t *h, uint32_t first, uint32_t n, psk_soft_frame_search_t *rec)
{
    if (!h || !rec || !n || !h->fsearch_called || (uint64_t)first + n > h->fsearch_n)
        return fail(PSK_SOFT_ERR_INVALID_ARG,
                    "psk_soft_get_frame_search: null pointer, no psk_soft_frame_search_device call yet or a range beyond its streams");
    return records_read(h, h->fsearch, h->fpass, first, n, rec);
}

// stream bit i of (bits, bit0)
static inline uint32_t frame_bit(const uint8_t *bits, uint64_t bit0, uint64_t i)
{
    const uint64_t g = bit0 + i;
    return (bits[g >> 3] >> (7u - (uint32_t)(g & 7u))) & 1u;
}

psk_soft_status psk_soft_frame_search_host(uint32_t length, uint64_t word, uint64_t care, const psk_soft_frame_search_in_t *in,
                                           psk_soft_frame_search_t *rec)
{
    if (!in || !rec || !psk::frame_word_ok(length, word, care))
        return fail(PSK_SOFT_ERR_INVALID_ARG, std::string("psk_soft_frame_search_host: ") + kFrameWordFault);
    *rec = psk_soft_frame_search_t{};
    if (frame_search_skipped(*in))
        return PSK_SOFT_OK;
    const uint32_t ncare = psk::frame_popcount(care);
    if (const char *what = frame_search_fault(*in, ncare))
        return fail(PSK_SOFT_ERR_INVALID_ARG, std::string("psk_soft_frame_search_host: ") + what);
    const uint32_t n_windows = frame_windows(in->n_bits, length), P = in->period;
    rec->flags = PSK_SOFT_FRAME_DATA, rec->length = length, rec->n_windows = n_windows;
    if (!n_windows)
        return PSK_SOFT_OK;
    const uint64_t keep = length == 64u ? ~0ull : (1ull << length) - 1ull;
    // one walk over the windows: the counts, the minimum, the score and the inverted hits of every phase; a second one lists
    uint64_t win = 0, min_key = ~0ull;
    for (uint32_t i = 0; i + 1u < length; i++) win = (win << 1) | frame_bit(in->bits, in->bit0, i);
    std::vector<uint32_t> score(P), inverted(P);
    for (uint32_t p = 0; p < n_windows; p++) {
        win = ((win << 1) | frame_bit(in->bits, in->bit0, (uint64_t)p + length - 1u)) & keep;
        const psk::FrameVerdict v = psk::frame_verdict(psk::frame_popcount((win ^ word) & care), ncare, in->max_diff);
        const uint64_t key = psk::frame_min_key(v.diff, p, v.pol);
        min_key = key < min_key ? key : min_key;
        if (!v.hit)
            continue;
        rec->n_hit[v.pol]++;
        if (P)
            score[p % P]++, inverted[p % P] += v.pol;
        else if (rec->n_listed < psk::kFrameHits)
            rec->hits[rec->n_listed++] = psk_soft_frame_hit_t{p, (uint16_t)v.diff, (uint8_t)v.pol, 0};
    }
    rec->min_diff = (uint32_t)(min_key >> 40), rec->min_pos = (uint32_t)(min_key >> 1) & 0x7fffffffu, rec->min_pol = (uint32_t)min_key & 1u;
    if (!P)
        return PSK_SOFT_OK;
    uint32_t best = 0;
    for (uint32_t f = 1; f < P; f++) best = score[f] > score[best] ? f : best;
    rec->best_phase = best, rec->best_score = score[best], rec->best_inv = inverted[best];
    for (uint64_t p = best; p < n_windows && rec->n_listed < psk::kFrameHits && score[best]; p += P) {
        uint64_t w = 0;
        for (uint32_t i = 0; i < length; i++) w = (w << 1) | frame_bit(in->bits, in->bit0, p + i);
        const psk::FrameVerdict v = psk::frame_verdict(psk::frame_popcount((w ^ word) & care), ncare, in->max_diff);
        if (v.hit)
            rec->hits[rec->n_listed++] = psk_soft_frame_hit_t{(uint32_t)p, (uint16_t)v.diff, (uint8_t)v.pol, 0};
    }
    return PSK_SOFT_OK;
}

uint32_t psk_soft_frame_tile(void) { return psk::kFrameTile; }

psk_soft_status psk_soft_frame_format_define(psk_soft_handle_t *h, uint32_t slot, uint32_t branches, uint32_t cell, const uint8_t *table)
{
    if (!h || slot >= psk::kFrameSlots || !psk::frame_format_ok(branches, cell))
        return fail(PSK_SOFT_ERR_INVALID_ARG, std::string("psk_soft_frame_format_define: ") + kFrameFormatFault);
    if (!h->dry) {
        PSK_HIP(hipSetDevice(h->device));
        PSK_TRY(h->cpass.wait());  // (no launch is still reading the slot)
        if (table) {
            if (!h->d_frame_tables)
                PSK_TRY(alloc_zeroed(h->d_frame_tables, (size_t)psk::kFrameSlots * 256u, "frame tables"));
            PSK_HIP(hipMemcpy(h->d_frame_tables + (size_t)slot * 256u, table, 256u, hipMemcpyHostToDevice));
        }
    }
    h->frame_format[slot] = psk::FrameFormat{branches, cell, table != nullptr};
    return PSK_SOFT_OK;
}

// what is wrong with a frame that is not skipped, cut with a format of `branches` branches; nullptr: nothing
static const char *frame_cut_fault(const psk_soft_frame_cut_in_t &k, uint32_t branches)
{
    if (k.branch0 >= branches)
        return "branch0 at or above the format's branches";
    if (k.n_bytes < 1u || k.n_bytes > psk::kFrameMaxBytes)
        return "n_bytes outside 1 .. 2^20";
    if (k.flags & ~psk::kFrameCutFlagMask)
        return "unknown flag bits";
    if (k.pad[0] || k.pad[1])
        return "pad must be zero";
    if (!k.out)
        return "out is null";
    return nullptr;
}

static const psk::FrameFormat kFramePlain = {1u, 0u, false};

psk_soft_status psk_soft_frame_cut_device(psk_soft_handle_t *h, uint32_t nframe, const psk_soft_frame_cut_in_t *in, void *stream_v)
{
    if (!h || !in || !nframe || nframe > psk::kFrameMaxFrames)
        return fail(PSK_SOFT_ERR_INVALID_ARG, "psk_soft_frame_cut_device: null pointer or a number of frames outside 1 .. 2^20");
    // the refusals, before anything is enqueued or any record changes
    for (uint32_t i = 0; i < nframe; i++) {
        const psk_soft_frame_cut_in_t &k = in[i];
        if (!k.bits)
            continue;
        const char *what = nullptr;
        if (k.format > psk::kFrameSlots || (k.format && !h->frame_format[k.format - 1u].branches))
            what = "a format slot above 15 or never defined (psk_soft_frame_format_define)";
        else
            what = frame_cut_fault(k, k.format ? h->frame_format[k.format - 1u].branches : 1u);
        if (what) {
            char buf[200];
            std::snprintf(buf, sizeof buf, "psk_soft_frame_cut_device: frame %u: %s", i, what);
            return fail(PSK_SOFT_ERR_INVALID_ARG, buf);
        }
    }
    if (h->dry) {
        h->fcut.dry.assign(nframe, psk_soft_frame_cut_t{});
        for (uint32_t i = 0; i < nframe; i++) {
            if (!in[i].bits)
                continue;
            const psk::FrameFormat &f = in[i].format ? h->frame_format[in[i].format - 1u] : kFramePlain;
            psk_soft_frame_cut_t &r = h->fcut.dry[i];
            r.n_bytes = in[i].n_bytes, r.span = psk::frame_span(f.branches, f.cell, in[i].branch0, in[i].n_bytes);
            r.flags = PSK_SOFT_FRAME_PLANNED | (in[i].flags << 1);
        }
        h->fcut_called = true, h->fcut_n = nframe;
        return PSK_SOFT_OK;
    }
    PSK_HIP(hipSetDevice(h->device));
    hipStream_t stream = stream_v ? (hipStream_t)stream_v : h->stream;
    // (a deferred call's classes end on the side streams: whatever made the bits must be complete)
    PSK_HIP(deferred_join(h, stream));
    const uint32_t grid = nframe < psk::kFrameCutGrid ? nframe : psk::kFrameCutGrid;
    PSK_TRY(h->fcut.grow(h->cpass, nframe));  // (the records are the last call's: nothing of them is kept)
    auto &q = h->cpass.next();
    PSK_TRY(h->cpass.claim(q, nframe, nframe / 4u + 256u));
    for (uint32_t i = 0; i < nframe; i++) {
        psk::FrameCutDesc &d = q.h_desc[i];
        d = psk::FrameCutDesc{};
        const psk_soft_frame_cut_in_t &k = in[i];
        if (!k.bits)
            continue;  // (its zero record)
        const psk::FrameFormat &f = k.format ? h->frame_format[k.format - 1u] : kFramePlain;
        // whole bytes of bit go into the pointer: the kernel counts bits in 32
        d.bits = k.bits + (k.bit >> 3), d.bit = k.bit & 7u, d.out = k.out;
        d.n_bytes = k.n_bytes, d.branches = f.branches, d.stride = psk::frame_stride(f.branches, f.cell), d.branch0 = k.branch0;
        d.flags = psk::kFrameData | (k.flags << 1);
        d.table = f.table ? k.format : 0u;
        d.span = psk::frame_span(f.branches, f.cell, k.branch0, k.n_bytes);
    }
    // (PSK_SOFT_TRACE_LAUNCHES, trace_launch: cnt = frames, tiles = workgroups)
    return h->cpass.run(q, nframe, kAllRecords, 0, stream, [&]() -> psk_soft_status {
        // the descriptors are up: the records are the new call's from here on, also if the launch below fails
        h->fcut_called = true, h->fcut_n = nframe;
        PSK_HIP(trace_launch(h, "frame_cut", 0, 0, 0, nframe, grid, 0, 0, h->slot, stream));
        PSK_HIP(psk::launch_frame_cut(q.d_desc, nframe, grid, h->d_frame_tables, h->fcut.d, stream));
        return PSK_SOFT_OK;
    });
}

psk_soft_status psk_soft_get_frame_cut(psk_soft_handle_t *h, uint32_t first, uint32_t n, psk_soft_frame_cut_t *rec)
{
    if (!h || !rec || !n || !h->fcut_called || (uint64_t)first + n > h->fcut_n)
        return fail(PSK_SOFT_ERR_INVALID_ARG,
                    "psk_soft_get_frame_cut: null pointer, no psk_soft_frame_cut_device call yet or a range beyond its frames");
    return records_read(h, h->fcut, h->cpass, first, n, rec);
}

psk_soft_status psk_soft_frame_cut_host(uint32_t branches, uint32_t cell, const uint8_t *table, const psk_soft_frame_cut_in_t *in,
                                        psk_soft_frame_cut_t *rec)
{
    if (!in || !rec || !psk::frame_format_ok(branches, cell))
        return fail(PSK_SOFT_ERR_INVALID_ARG, std::string("psk_soft_frame_cut_host: ") + kFrameFormatFault);
    *rec = psk_soft_frame_cut_t{};
    if (!in->bits)
        return PSK_SOFT_OK;
    if (const char *what = frame_cut_fault(*in, branches))
        return fail(PSK_SOFT_ERR_INVALID_ARG, std::string("psk_soft_frame_cut_host: ") + what);
    const uint32_t stride = psk::frame_stride(branches, cell);
    const uint32_t inv = (in->flags & PSK_SOFT_FRAME_INVERT) ? 0xffu : 0u;
    uint32_t ones = 0;
    for (uint32_t i = 0; i < in->n_bytes; i++) {
        const uint64_t q = psk::frame_source(i, in->branch0, branches, stride);
        uint32_t b = 0;
        for (uint32_t j = 0; j < 8u; j++) b = (b << 1) | frame_bit(in->bits, in->bit, 8u * q + j);
        b ^= inv;
        b = table ? table[b] : b;
        in->out[i] = (uint8_t)b;
        ones += psk::frame_popcount(b);
    }
    rec->flags = PSK_SOFT_FRAME_DATA | (in->flags << 1);
    rec->n_bytes = in->n_bytes, rec->span = psk::frame_span(branches, cell, in->branch0, in->n_bytes), rec->n_ones = ones;
    return PSK_SOFT_OK;
}

uint64_t psk_soft_frame_span(uint32_t branches, uint32_t cell, uint32_t branch0, uint32_t n_bytes)
{
    if (!psk::frame_format_ok(branches, cell) || branch0 >= branches || n_bytes < 1u || n_bytes > psk::kFrameMaxBytes)
        return 0;
    return psk::frame_span(branches, cell, branch0, n_bytes);
}

uint64_t psk_soft_frame_search_bytes(void) { return sizeof(psk_soft_frame_search_t); }
uint64_t psk_soft_frame_search_in_bytes(void) { return sizeof(psk_soft_frame_search_in_t); }
uint64_t psk_soft_frame_cut_bytes(void) { return sizeof(psk_soft_frame_cut_t); }
uint64_t psk_soft_frame_cut_in_bytes(void) { return sizeof(psk_soft_frame_cut_in_t); }
static_assert(sizeof(psk_soft_frame_search_t) == 192 && sizeof(psk_soft_frame_search_in_t) == 48 && sizeof(psk_soft_frame_cut_t) == 32 &&
                  sizeof(psk_soft_frame_cut_in_t) == 48 && sizeof(psk_soft_frame_hit_t) == 8,
              "include/psk_soft_frame.h states the sizes");
static_assert(offsetof(psk_soft_frame_search_t, n_hit) == 12 && offsetof(psk_soft_frame_search_t, min_diff) == 20 &&
                  offsetof(psk_soft_frame_search_t, best_phase) == 32 && offsetof(psk_soft_frame_search_t, n_listed) == 44 &&
                  offsetof(psk_soft_frame_search_t, hits) == 64 && offsetof(psk_soft_frame_hit_t, diff) == 4 &&
                  offsetof(psk_soft_frame_hit_t, pol) == 6,
              "psk_frame.hip stores the search record as sixteen words and sixteen hits");
static_assert(offsetof(psk_soft_frame_cut_t, span) == 8 && offsetof(psk_soft_frame_cut_t, n_ones) == 12,
              "psk_frame.hip stores the cut record as eight words");
static_assert(PSK_SOFT_FRAME_DATA == psk::kFrameData && PSK_SOFT_FRAME_REC_INVERT == PSK_SOFT_FRAME_INVERT << 1,
              "the cut record's flags are the frame's shifted left by one");

// ---- host-buffer path: the ingest pipeline --------------------------
// The batch is cut into chunks of channels of about `stage_bytes` of input each.  Per chunk: the
// packets are packed into pinned memory (CopyPool), uploaded with ONE copy, processed, and the four
// output streams -- packed tightly, their sizes are known from the plan -- come back with one copy
// each and are scattered to the caller's buffers.  kStageSlots chunks are in flight on separate
// streams, so upload, kernels, download and the two host-side copies of different chunks overlap.
static psk_soft_status stage_ensure(psk_soft_handle *h, StageSlot &sl, size_t in_bytes)
{
    if (!sl.stream) {
        PSK_HIP(sl.stream.create());
        PSK_HIP(sl.done.ensure());
    }
    if (sl.in_cap >= in_bytes)
        return PSK_SOFT_OK;
    size_t cap = align_up(in_bytes > h->stage_bytes ? in_bytes : h->stage_bytes, 4096);
    sl.h_buf.release(), sl.d_buf.release();
    sl.in_cap = 0;
    PSK_HIP(sl.h_buf.alloc(region_total(cap)));
    PSK_HIP(sl.d_buf.alloc(region_total(cap)));
    sl.in_cap = cap;
    return PSK_SOFT_OK;
}

// results of the chunk in `sl` -> the caller's buffers
static psk_soft_status stage_retire(psk_soft_handle *h, StageSlot &sl, psk_soft_output_t *outs, uint32_t batch_ch0)
{
    if (!sl.busy)
        return PSK_SOFT_OK;
    PSK_HIP(sl.done.sync());
    const uint8_t *hs = sl.h_buf + region_soft(sl.in_cap), *hp = sl.h_buf + region_phase(sl.in_cap);
    const uint8_t *hb = sl.h_buf + region_bits(sl.in_cap), *hx = sl.h_buf + region_sidx(sl.in_cap);
    psk_soft_output_t *o0 = outs + (sl.ch0 - batch_ch0);
    h->pool->run(sl.nch, [&](uint32_t i) {
        const psk_soft_output_t &o = o0[i];
        if (!o.n_symbols)
            return;
        if (o.soft) std::memcpy(o.soft, hs + sl.off_soft[i], sizeof(float) * 2 * o.n_symbols);
        if (o.phase) std::memcpy(o.phase, hp + sl.off_phase[i], sizeof(float) * o.n_symbols);
        if (o.bits && o.n_bits) std::memcpy(o.bits, hb + sl.off_bits[i], sizeof(int16_t) * o.n_bits);
        if (o.sampleIndex && o.n_sampleIndex) std::memcpy(o.sampleIndex, hx + sl.off_sidx[i], sizeof(int16_t) * o.n_sampleIndex);
    });
    sl.busy = false;
    return PSK_SOFT_OK;
}

psk_soft_status psk_soft_process_host(psk_soft_handle_t *h, uint32_t ch0, uint32_t nch, const psk_soft_packet_t *pkts,
                                      psk_soft_output_t *outs)
{
    if (!h || !pkts || !outs || !nch || (uint64_t)ch0 + nch > h->nch)
        return fail(PSK_SOFT_ERR_INVALID_ARG, "psk_soft_process_host: bad arguments");
    if (h->dry) {
        std::vector<psk_soft_packet_t> pk(pkts, pkts + nch);
        return psk_soft_process_device(h, ch0, nch, pk.data(), outs, nullptr);
    }
    PSK_HIP(hipSetDevice(h->device));
    if (!h->pool) {
        int nt = 8;
        if (const char *e = std::getenv("PSK_SOFT_HOST_THREADS")) nt = std::atoi(e);
        unsigned hw = std::thread::hardware_concurrency();
        if (hw && (unsigned)nt > hw) nt = (int)hw;
        h->pool.reset(new CopyPool(nt > 1 ? nt - 1 : 0));  // the calling thread works too
        if (const char *e = std::getenv("PSK_SOFT_STAGE_MB")) {
            long mb = std::atol(e);
            if (mb >= 1 && mb <= 4096) h->stage_bytes = (size_t)mb << 20;
        }
    }
    // validate the whole batch first (all or nothing, as psk_soft_process_device), and learn the
    // output sizes: they depend only on packet sizes and properties
    struct Need {
        size_t in, soft, phase, bits, sidx;
    };
    std::vector<Need> need(nch);
    ctl_sync(h);
    for (uint32_t i = 0; i < nch; i++) {
        if (pkts[i].present && pkts[i].n_floats / 2 > h->user.max_packet_complex)
            return fail(PSK_SOFT_ERR_LIMIT, "psk_soft_process_host: packet longer than max_packet_complex");
        if (pkts[i].present && pkts[i].n_floats && !pkts[i].data)
            return fail(PSK_SOFT_ERR_INVALID_ARG, "psk_soft_process_host: null packet data");
        psk::ChanCtl probe = h->ctl[ch0 + i];
        psk::ChanPlan pl;
        psk_soft_output_t o = outs[i];
        o.cap_symbols = ~0ull;
        psk_soft_status st = psk::plan_call(probe, h->lim, pkts[i], o, pl);
        if (st != PSK_SOFT_OK) {
            char buf[160];
            std::snprintf(buf, sizeof buf, "psk_soft_process_host: channel %u refused (status %d)", ch0 + i, (int)st);
            return fail(st, buf);
        }
        if (o.n_symbols > outs[i].cap_symbols && (outs[i].soft || outs[i].bits || outs[i].phase || outs[i].sampleIndex))  // (plan_call's rule)
            return fail(PSK_SOFT_ERR_CAPACITY, "psk_soft_process_host: output buffer too small");
        // every channel's rows start on a cache line: rows that straddle lines cost 6-8 % of the
        // kernel's streaming rate (tools/micro/placement_probe.hip)
        need[i].in = pkts[i].present ? align_up(elem_bytes(pkts[i]) * (pkts[i].n_floats & ~1ull), 128) : 0;  // (CS16 / CS8 / CF16 staged as such)
        need[i].soft = align_up(sizeof(float) * 2 * o.n_symbols, 128);
        need[i].phase = align_up(sizeof(float) * o.n_symbols, 128);
        need[i].bits = align_up(sizeof(int16_t) * o.n_bits, 128);
        need[i].sidx = align_up(sizeof(int16_t) * o.n_sampleIndex, 128);
    }
    std::vector<psk_soft_packet_t> dp;
    std::vector<psk_soft_output_t> dout;
    uint32_t first = 0;
    int turn = 0;
    psk_soft_status status = PSK_SOFT_OK;
    while (first < nch && status == PSK_SOFT_OK) {
        // chunk [first, last): as many channels as fit the five regions of a slot
        Need sum = {0, 0, 0, 0, 0};
        const size_t cap = h->stage_bytes;
        uint32_t last = first;
        while (last < nch) {
            const Need &n = need[last];
            if (last > first && (sum.in + n.in > cap || sum.soft + n.soft > cap || sum.phase + n.phase > cap / 2 ||
                                 sum.bits + n.bits > cap || sum.sidx + n.sidx > cap / 4))
                break;
            sum.in += n.in;
            sum.soft += n.soft;
            sum.phase += n.phase;
            sum.bits += n.bits;
            sum.sidx += n.sidx;
            last++;
        }
        // a single oversized packet gets a slot grown to fit it
        size_t want = sum.in;
        if (sum.soft > want) want = sum.soft;
        if (2 * sum.phase > want) want = 2 * sum.phase;
        if (sum.bits > want) want = sum.bits;
        if (4 * sum.sidx > want) want = 4 * sum.sidx;
        StageSlot &sl = h->stage[turn];
        turn = (turn + 1) % kStageSlots;
        if ((status = stage_retire(h, sl, outs, ch0)) != PSK_SOFT_OK)
            break;
        if ((status = stage_ensure(h, sl, want)) != PSK_SOFT_OK)
            break;
        const uint32_t n = last - first;
        sl.ch0 = ch0 + first;
        sl.nch = n;
        sl.off_soft.resize(n);
        sl.off_phase.resize(n);
        sl.off_bits.resize(n);
        sl.off_sidx.resize(n);
        dp.assign(pkts + first, pkts + last);
        dout.assign(outs + first, outs + last);
        std::vector<size_t> off_in(n);
        size_t oi = 0, os = 0, op = 0, ob = 0, ox = 0;
        uint8_t *d_in = sl.d_buf, *d_soft = sl.d_buf + region_soft(sl.in_cap), *d_phase = sl.d_buf + region_phase(sl.in_cap);
        uint8_t *d_bits = sl.d_buf + region_bits(sl.in_cap), *d_sidx = sl.d_buf + region_sidx(sl.in_cap);
        for (uint32_t i = 0; i < n; i++) {
            const Need &nd = need[first + i];
            off_in[i] = oi;
            sl.off_soft[i] = os;
            sl.off_phase[i] = op;
            sl.off_bits[i] = ob;
            sl.off_sidx[i] = ox;
            dp[i].data = (const float *)(d_in + oi);
            dout[i].soft = (float *)(d_soft + os);
            dout[i].phase = (float *)(d_phase + op);
            dout[i].bits = (int16_t *)(d_bits + ob);
            dout[i].sampleIndex = (int16_t *)(d_sidx + ox);
            dout[i].cap_symbols = ~0ull;
            oi += nd.in;
            os += nd.soft;
            op += nd.phase;
            ob += nd.bits;
            ox += nd.sidx;
        }
        sl.soft_bytes = os;
        sl.phase_bytes = op;
        sl.bits_bytes = ob;
        sl.sidx_bytes = ox;
        // pack, upload, process, download
        const psk_soft_packet_t *pk0 = pkts + first;
        uint8_t *h_in = sl.h_buf;
        h->pool->run(n, [&](uint32_t i) {
            if (pk0[i].present && pk0[i].n_floats)
                std::memcpy(h_in + off_in[i], pk0[i].data, elem_bytes(pk0[i]) * (pk0[i].n_floats & ~1ull));
        });
        if (oi)
            PSK_HIP(hipMemcpyAsync(d_in, h_in, oi, hipMemcpyHostToDevice, sl.stream));
        status = psk_soft_process_device(h, ch0 + first, n, dp.data(), dout.data(), sl.stream);
        if (status == PSK_SOFT_OK)  // (deferred join: the downloads below read what the side streams write)
            PSK_HIP(deferred_join(h, sl.stream));
        if (status != PSK_SOFT_OK)
            break;
        for (uint32_t i = 0; i < n; i++) {
            psk_soft_output_t &o = outs[first + i];
            const psk_soft_output_t &d = dout[i];
            o.ret = d.ret;
            o.n_symbols = d.n_symbols;
            o.n_bits = d.n_bits;
            o.n_sampleIndex = d.n_sampleIndex;
            o.sri_pushed = d.sri_pushed;
            o.sri_soft_xdelta = d.sri_soft_xdelta;
            o.sri_bits_xdelta = d.sri_bits_xdelta;
            o.n_warn = d.n_warn;
        }
        if (os) PSK_HIP(hipMemcpyAsync(sl.h_buf + region_soft(sl.in_cap), d_soft, os, hipMemcpyDeviceToHost, sl.stream));
        if (op) PSK_HIP(hipMemcpyAsync(sl.h_buf + region_phase(sl.in_cap), d_phase, op, hipMemcpyDeviceToHost, sl.stream));
        if (ob) PSK_HIP(hipMemcpyAsync(sl.h_buf + region_bits(sl.in_cap), d_bits, ob, hipMemcpyDeviceToHost, sl.stream));
        if (ox) PSK_HIP(hipMemcpyAsync(sl.h_buf + region_sidx(sl.in_cap), d_sidx, ox, hipMemcpyDeviceToHost, sl.stream));
        PSK_HIP(sl.done.record(sl.stream));
        sl.busy = true;
        first = last;
    }
    // drain, oldest first
    for (int k = 0; k < kStageSlots; k++) {
        psk_soft_status st = stage_retire(h, h->stage[(turn + k) % kStageSlots], outs, ch0);
        if (status == PSK_SOFT_OK)
            status = st;
    }
    return status;
}

psk_soft_status psk_soft_synchronize(psk_soft_handle_t *h)
{
    if (!h)
        return fail(PSK_SOFT_ERR_INVALID_ARG, "null handle");
    if (h->dry)
        return PSK_SOFT_OK;
    PSK_HIP(hipSetDevice(h->device));
    for (const Event &e : h->ev) PSK_HIP(e.sync());
    PSK_HIP(h->stream.sync());
    for (const Stream &s : h->aux) PSK_HIP(s.sync());
    if (h->deferred_pending && h->deferred_stream)
        PSK_HIP(hipStreamSynchronize(h->deferred_stream));
    h->deferred_pending = false;
    for (auto &row : h->slot_aux_ev)
        for (Event &e : row) e.clear();
    for (const StageSlot &sl : h->stage) PSK_HIP(sl.stream.sync());
    return PSK_SOFT_OK;
}

psk_soft_status psk_soft_join(psk_soft_handle_t *h, void *stream_v)
{
    if (!h)
        return fail(PSK_SOFT_ERR_INVALID_ARG, "null handle");
    if (h->dry || !h->deferred_pending)
        return PSK_SOFT_OK;
    PSK_HIP(hipSetDevice(h->device));
    hipStream_t stream = stream_v ? (hipStream_t)stream_v : h->stream;
    // (the caller's stream of the deferred calls carries one class itself: a third stream waits for it too)
    if (h->deferred_stream && h->deferred_stream != stream) {
        if (!h->aux_fork)
            return PSK_SOFT_OK;
        PSK_HIP(h->aux_fork.record(h->deferred_stream));
        PSK_HIP(h->aux_fork.wait(stream));
    }
    h->deferred_pending = true;  // (deferred_join() clears it)
    PSK_HIP(deferred_join(h, stream));
    return PSK_SOFT_OK;
}

static void stats_add(psk_soft_stats_t *stats, uint32_t mode, const psk::ChanState &s)
{
    switch (mode) {
    case psk::PLAN_FAST:
        if (s.guard == 2u) {
            stats->channels_sequential++;
            stats->channels_guard++;
        } else {
            stats->channels_fast++;
            if (s.guard == 3u)
                stats->channels_exact_timing++;
            if (s.guard == 4u) {
                stats->channels_tiled++;
                if (s.stat_pfit & 1u) {
                    stats->channels_parallel_fit++;
                    if (s.stat_pfit & 0x100u)
                        stats->channels_parallel_fit_second_round++;
                } else {
                    stats->parallel_fit_refusals |= s.stat_pfit >> 1;
                }
            }
            stats->unwrap_blocks += s.stat_blocks;
            stats->unwrap_extra_passes += s.stat_extra;
            stats->timing_exact_blocks += s.stat_exact;
            stats->fit_chain_blocks += s.stat_chain;
        }
        break;
    case psk::PLAN_SEQ:
    case psk::PLAN_SEQ_S1: stats->channels_sequential++; break;
    default: break;
    }
}

static psk_soft_status stats_range(psk_soft_handle_t *h, uint32_t ch0, uint32_t nch, psk_soft_stats_t *stats, bool per_channel)
{
    if (!h || !stats || (uint64_t)ch0 + nch > h->nch)
        return fail(PSK_SOFT_ERR_INVALID_ARG, "psk_soft_get_stats: bad arguments");
    ctl_sync(h);
    std::memset(stats, 0, sizeof *stats * (per_channel ? nch : 1));
    if (h->dry) {  // control plane only: which kernel the last call was PLANNED for, per channel
        for (uint32_t c = 0; c < nch; c++) {
            psk_soft_stats_t *o = per_channel ? stats + c : stats;
            if (h->last_mode[ch0 + c] == psk::PLAN_FAST) o->channels_fast++;
            if (h->last_mode[ch0 + c] == psk::PLAN_SEQ || h->last_mode[ch0 + c] == psk::PLAN_SEQ_S1) o->channels_sequential++;
        }
        return PSK_SOFT_OK;
    }
    psk_soft_status st = psk_soft_synchronize(h);
    if (st != PSK_SOFT_OK)
        return st;
    std::vector<psk::ChanState> s(nch);
    PSK_HIP(hipMemcpy(s.data(), h->d_state + ch0, sizeof(psk::ChanState) * nch, hipMemcpyDeviceToHost));
    for (uint32_t c = 0; c < nch; c++) stats_add(per_channel ? stats + c : stats, h->last_mode[ch0 + c], s[c]);
    return PSK_SOFT_OK;
}

psk_soft_status psk_soft_get_stats(psk_soft_handle_t *h, psk_soft_stats_t *stats)
{
    return stats_range(h, 0, h ? h->nch : 0, stats, false);
}

psk_soft_status psk_soft_get_channel_stats(psk_soft_handle_t *h, uint32_t ch0, uint32_t nch, psk_soft_stats_t *stats)
{
    return stats_range(h, ch0, nch, stats, true);
}

// everything enqueued so far, the quality passes behind the calls included
static psk_soft_status quality_wait(psk_soft_handle_t *h)
{
    const psk_soft_status st = psk_soft_synchronize(h);
    if (st != PSK_SOFT_OK)
        return st;
    return h->qpass.wait();
}

uint64_t psk_soft_quality_bytes(void) { return sizeof(psk_soft_quality_t); }

psk_soft_status psk_soft_get_quality(psk_soft_handle_t *h, uint32_t ch0, uint32_t nch, psk_soft_quality_t *q)
{
    if (!h || !q || !nch || (uint64_t)ch0 + nch > h->nch)
        return fail(PSK_SOFT_ERR_INVALID_ARG, "psk_soft_get_quality: bad arguments");
    return records_read(h, h->quality, h->qpass, ch0, nch, q);
}

psk_soft_status psk_soft_quality_derive(const psk_soft_quality_t *q, psk_soft_quality_derived_t *d)
{
    if (!q || !d)
        return fail(PSK_SOFT_ERR_INVALID_ARG, "psk_soft_quality_derive: null pointer");
    const double nan = std::nan("");
    d->lock = d->snr_db = d->mean_energy = d->index_change_rate = nan;
    if ((q->flags & PSK_SOFT_Q_LOCK) && q->n_lock)
        d->lock = std::hypot(q->sum_lock_re, q->sum_lock_im) / (double)q->n_lock;
    if (q->n_finite) {
        const double m2 = q->sum_e / (double)q->n_finite, m4 = q->sum_e2 / (double)q->n_finite;
        d->mean_energy = m2;
        const double dd = 2.0 * m2 * m2 - m4;
        if (!q->differentialDecoding && dd > 0.0) {
            const double s = std::sqrt(dd);
            if (m2 - s > 0.0)
                d->snr_db = 10.0 * std::log10(s / (m2 - s));
        }
    }
    if ((q->flags & PSK_SOFT_Q_INDEX) && q->n_symbols >= 2)
        d->index_change_rate = (double)q->index_changes / (double)(q->n_symbols - 1);
    return PSK_SOFT_OK;
}

psk_soft_status psk_soft_set_option(psk_soft_handle_t *h, int option, int value)
{
    if (!h)
        return fail(PSK_SOFT_ERR_INVALID_ARG, "null handle");
    switch (option) {
    case PSK_SOFT_OPT_QPSK_SIGN_BITMAP: h->opt_qpsk_sign_map = value != 0; return PSK_SOFT_OK;
    case PSK_SOFT_OPT_CONCURRENT_CLASSES: h->opt_fork = value != 0; return PSK_SOFT_OK;
    case PSK_SOFT_OPT_DEFERRED_JOIN:
        if (!value && h->deferred_pending && !h->dry) {
            const psk_soft_status st = psk_soft_synchronize(h);
            if (st != PSK_SOFT_OK)
                return st;
        }
        h->opt_deferred = value != 0;
        return PSK_SOFT_OK;
    case PSK_SOFT_OPT_TIME_TILED:
        if (value < 0 || value > 2)
            return fail(PSK_SOFT_ERR_INVALID_ARG, "psk_soft_set_option: PSK_SOFT_OPT_TIME_TILED takes 0, 1 or 2");
        h->opt_tiled = value;
        return PSK_SOFT_OK;
    case PSK_SOFT_OPT_PARALLEL_FIT:
        if (value < 0 || value > 2)
            return fail(PSK_SOFT_ERR_INVALID_ARG, "psk_soft_set_option: PSK_SOFT_OPT_PARALLEL_FIT takes 0, 1 or 2");
        h->opt_pfit = value;
        return PSK_SOFT_OK;
    case PSK_SOFT_OPT_QUALITY:
        if (value != 0 && value != 1)
            return fail(PSK_SOFT_ERR_INVALID_ARG, "psk_soft_set_option: PSK_SOFT_OPT_QUALITY takes 0 or 1");
        if (value) {  // (all records zeroed)
            if (h->dry) {
                h->quality.dry.assign(h->nch, psk_soft_quality_t{});
            } else {
                const psk_soft_status st = quality_wait(h);
                if (st != PSK_SOFT_OK)
                    return st;
                PSK_HIP(hipMemset(h->quality.d, 0, sizeof(psk_soft_quality_t) * (size_t)h->nch));
            }
        }
        h->opt_quality = value;
        return PSK_SOFT_OK;
    case PSK_SOFT_OPT_FAR_FIT:
        if (value != 0 && value != 1)
            return fail(PSK_SOFT_ERR_INVALID_ARG, "psk_soft_set_option: PSK_SOFT_OPT_FAR_FIT takes 0 or 1");
        h->opt_far_fit = value;
        h->lim.far_fit = value != 0;  // (process_round reads the limits once per call: from the next call on)
        return PSK_SOFT_OK;
    default: return fail(PSK_SOFT_ERR_INVALID_ARG, "psk_soft_set_option: unknown option");
    }
}

psk_soft_status psk_soft_set_force_sequential(psk_soft_handle_t *h, int on)
{
    if (!h)
        return fail(PSK_SOFT_ERR_INVALID_ARG, "null handle");
    h->lim.force_seq = on != 0;
    return PSK_SOFT_OK;
}

// A saved channel state: header, control-plane mirror, device state, sample ring (the current buffer), phase history.
struct StateHeader {
    uint32_t magic, version;      // "PSKS", PSK_SOFT_ABI_VERSION
    uint32_t ring_cap, fit_cap;   // the limits the blob was written under: they size its two arrays
    uint32_t ctl_bytes, state_bytes;
};
constexpr uint32_t kStateMagic = 0x534B5350u;  // 'P' 'S' 'K' 'S'

uint64_t psk_soft_state_bytes(const psk_soft_handle_t *h)
{
    if (!h)
        return 0;
    return sizeof(StateHeader) + sizeof(psk::ChanCtl) + sizeof(psk::ChanState) + sizeof(float2) * (uint64_t)h->lim.ring_cap +
           sizeof(float) * (uint64_t)h->lim.fit_cap;
}

psk_soft_status psk_soft_export_state(psk_soft_handle_t *h, uint32_t ch, void *dst, uint64_t cap)
{
    if (!h || !dst || ch >= h->nch || cap < psk_soft_state_bytes(h))
        return fail(PSK_SOFT_ERR_INVALID_ARG, "psk_soft_export_state: bad arguments");
    ctl_sync(h);
    uint8_t *p = (uint8_t *)dst;
    std::memset(p, 0, psk_soft_state_bytes(h));
    StateHeader hd = {kStateMagic, PSK_SOFT_ABI_VERSION, h->lim.ring_cap, h->lim.fit_cap, (uint32_t)sizeof(psk::ChanCtl),
                      (uint32_t)sizeof(psk::ChanState)};
    std::memcpy(p, &hd, sizeof hd);
    p += sizeof hd;
    std::memcpy(p, &h->ctl[ch], sizeof(psk::ChanCtl));
    p += sizeof(psk::ChanCtl);
    if (h->dry)
        return PSK_SOFT_OK;
    psk_soft_status st = psk_soft_synchronize(h);
    if (st != PSK_SOFT_OK)
        return st;
    PSK_HIP(hipMemcpy(p, h->d_state + ch, sizeof(psk::ChanState), hipMemcpyDeviceToHost));
    p += sizeof(psk::ChanState);
    const float2 *ring = h->d_ring + ((size_t)ch * 2 + h->ctl[ch].ring_src) * h->lim.ring_cap;
    PSK_HIP(hipMemcpy(p, ring, sizeof(float2) * h->lim.ring_cap, hipMemcpyDeviceToHost));
    p += sizeof(float2) * h->lim.ring_cap;
    PSK_HIP(hipMemcpy(p, h->d_yv + (size_t)ch * h->lim.fit_cap, sizeof(float) * h->lim.fit_cap, hipMemcpyDeviceToHost));
    return PSK_SOFT_OK;
}

psk_soft_status psk_soft_import_state(psk_soft_handle_t *h, uint32_t ch, const void *src, uint64_t bytes)
{
    if (!h || !src || ch >= h->nch || bytes != psk_soft_state_bytes(h))
        return fail(PSK_SOFT_ERR_INVALID_ARG, "psk_soft_import_state: bad arguments (the blob must be exactly psk_soft_state_bytes long)");
    const uint8_t *p = (const uint8_t *)src;
    StateHeader hd;
    std::memcpy(&hd, p, sizeof hd);
    p += sizeof hd;
    if (hd.magic != kStateMagic || hd.version != PSK_SOFT_ABI_VERSION || hd.ring_cap != h->lim.ring_cap ||
        hd.fit_cap != h->lim.fit_cap || hd.ctl_bytes != sizeof(psk::ChanCtl) || hd.state_bytes != sizeof(psk::ChanState))
        return fail(PSK_SOFT_ERR_INVALID_ARG, "psk_soft_import_state: not a state blob of this library version and these limits");
    // everything the kernels use as an index is checked before anything is overwritten
    psk::ChanCtl c;
    std::memcpy(static_cast<void *>(&c), p, sizeof c);
    p += sizeof c;
    if (c.ring_src > 1u || c.lf_head >= h->lim.fit_cap || c.lf_len > c.lf_n || c.lf_n >= h->lim.fit_cap || c.lf_len >= h->lim.fit_cap ||
        c.lf_count > psk::kResyncCount || c.count > psk::kResyncCount ||
        (uint64_t)c.props.samplesPerBaud * c.props.numAvg > h->lim.ring_cap || c.props.phaseAvg >= h->lim.fit_cap)
        return fail(PSK_SOFT_ERR_INVALID_ARG, "psk_soft_import_state: control state out of range for this handle");
    if (!h->dry) {
        psk_soft_status st = psk_soft_synchronize(h);
        if (st != PSK_SOFT_OK)
            return st;
        PSK_HIP(hipSetDevice(h->device));
        PSK_HIP(hipMemcpy(h->d_state + ch, p, sizeof(psk::ChanState), hipMemcpyHostToDevice));
        p += sizeof(psk::ChanState);
        float2 *ring = h->d_ring + ((size_t)ch * 2 + c.ring_src) * h->lim.ring_cap;
        PSK_HIP(hipMemcpy(ring, p, sizeof(float2) * h->lim.ring_cap, hipMemcpyHostToDevice));
        p += sizeof(float2) * h->lim.ring_cap;
        PSK_HIP(hipMemcpy(h->d_yv + (size_t)ch * h->lim.fit_cap, p, sizeof(float) * h->lim.fit_cap, hipMemcpyHostToDevice));
    }
    c.pad_flags = 0, c.pad_rate = 0, c.pad_xdelta = 0;  // (a blob of an earlier build may hold indeterminate bytes there)
    std::memset(c.pad_tail, 0, sizeof c.pad_tail);
    ctl_touch(h);
    h->ctl[ch] = c;  // (last: a failed copy above leaves the host mirror as it was)
    return PSK_SOFT_OK;
}

psk_soft_status psk_soft_probe_read_ms(psk_soft_handle_t *h, const void *dev_ptr, uint64_t bytes, int reps,
                                       double *ms_per_pass)
{
    if (!h || h->dry || !dev_ptr || bytes < 16 || ((uintptr_t)dev_ptr & 15u) || reps < 1 || !ms_per_pass)
        return fail(PSK_SOFT_ERR_INVALID_ARG, "psk_soft_probe_read_ms: needs a device handle, a 16-byte aligned device "
                                              "pointer, at least 16 bytes and one repetition");
    PSK_HIP(hipSetDevice(h->device));
    Event e0, e1;  // (with timing; they go on every way out)
    PSK_HIP(e0.ensure(true));
    PSK_HIP(e1.ensure(true));
    float *sink = reinterpret_cast<float *>(h->d_state.get());  // (never written: see the kernel)
    PSK_HIP(psk::launch_read_probe(dev_ptr, bytes, sink, h->stream));  // untimed first pass
    PSK_HIP(e0.record(h->stream));
    for (int r = 0; r < reps; r++) PSK_HIP(psk::launch_read_probe(dev_ptr, bytes, sink, h->stream));
    PSK_HIP(e1.record(h->stream));
    PSK_HIP(e1.sync());
    float ms = 0.0f;
    PSK_HIP(hipEventElapsedTime(&ms, e0.get(), e1.get()));
    *ms_per_pass = (double)ms / reps;
    return PSK_SOFT_OK;
}

void *psk_soft_host_alloc(size_t bytes)
{
    void *p = nullptr;
    if (!bytes || hipHostMalloc(&p, bytes, hipHostMallocDefault) != hipSuccess) {
        g_last_error = "psk_soft_host_alloc: hipHostMalloc failed";
        return nullptr;
    }
    return p;
}

void psk_soft_host_free(void *p)
{
    if (p)
        (void)hipHostFree(p);
}

void *psk_soft_device_alloc(psk_soft_handle_t *h, size_t bytes)
{
    void *p = nullptr;
    if (!h || h->dry || !bytes || hipSetDevice(h->device) != hipSuccess || hipMalloc(&p, bytes) != hipSuccess) {
        g_last_error = "psk_soft_device_alloc: needs a device handle and a size; or hipMalloc failed";
        return nullptr;
    }
    return p;
}

void psk_soft_device_free(psk_soft_handle_t *h, void *p)
{
    if (h && !h->dry && p && hipSetDevice(h->device) == hipSuccess)
        (void)hipFree(p);
}

psk_soft_status psk_soft_device_upload(psk_soft_handle_t *h, void *dev_dst, const void *host_src, size_t bytes)
{
    if (!h || h->dry || !dev_dst || !host_src)
        return fail(PSK_SOFT_ERR_INVALID_ARG, "psk_soft_device_upload: bad arguments");
    PSK_HIP(hipSetDevice(h->device));
    PSK_HIP(hipMemcpy(dev_dst, host_src, bytes, hipMemcpyHostToDevice));
    return PSK_SOFT_OK;
}

psk_soft_status psk_soft_device_download(psk_soft_handle_t *h, void *host_dst, const void *dev_src, size_t bytes)
{
    if (!h || h->dry || !host_dst || !dev_src)
        return fail(PSK_SOFT_ERR_INVALID_ARG, "psk_soft_device_download: bad arguments");
    PSK_HIP(hipSetDevice(h->device));
    PSK_HIP(hipMemcpy(host_dst, dev_src, bytes, hipMemcpyDeviceToHost));
    return PSK_SOFT_OK;
}

psk_soft_status psk_soft_peek(const psk_soft_handle_t *h, uint32_t ch, uint64_t *ring_len, uint64_t *index,
                              uint64_t *fit_len)
{
    if (!h || ch >= h->nch)
        return fail(PSK_SOFT_ERR_INVALID_ARG, "psk_soft_peek: bad channel");
    ctl_sync(h);
    if (ring_len) *ring_len = h->ctl[ch].ring_len;
    if (index) *index = h->ctl[ch].index;
    if (fit_len) *fit_len = h->ctl[ch].lf_len;
    return PSK_SOFT_OK;
}

}  // extern "C"
#undef PSK_TRY
