/*
 * psk_soft_hip.h -- C ABI of libpsk_soft_hip.so, the MI355X (gfx950) implementation of
 * the hot path of REDHAWK rh.psk_soft.
 *
 * Drop-in boundary.  The library replaces, inside
 * psk_soft_i::serviceFunction(), everything from the reinterpretation of the
 * packet as complex samples to the end-of-call phase wrap
 *     reference cpp/psk_soft.cpp:365-603   (flag handling, resyncEnergy, LinearFit
 *                                           resets, the per-sample / per-symbol loop,
 *                                           the end-of-call wrap)
 *     reference cpp/psk_soft.cpp:35-185    (class LinearFit)
 *     reference cpp/psk_soft.cpp:619-651   (resyncEnergy, property listeners)
 * and leaves on the C++ host: getPacket / delete (:349-352, :616), the pushSRI and
 * pushPacket calls (:400-404, :605-615).  The host keeps calling it from the one
 * service thread REDHAWK gives the component.
 *
 * One "channel" = the complete state of one psk_soft_i instance (one stream).
 * Channels are independent; a handle owns a batch of them on ONE GPU.  All
 * functions return a psk_soft_status, never throw, never call back.  Caller owns
 * every buffer passed in for the duration of the call; the library owns the
 * per-channel demodulator state, which lives in HBM between calls.
 *
 * Plain pointers and sizes only -- no C++ or torch types cross this boundary.
 */
#ifndef PSK_SOFT_HIP_H
#define PSK_SOFT_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PSK_SOFT_ABI_VERSION 2

typedef enum psk_soft_status {
    PSK_SOFT_OK = 0,
    PSK_SOFT_ERR_INVALID_ARG = 1,
    PSK_SOFT_ERR_NO_DEVICE = 2,     /* no usable gfx950 device / HIP runtime error at create */
    PSK_SOFT_ERR_HIP = 3,           /* a HIP call failed; see psk_soft_last_error()          */
    PSK_SOFT_ERR_LIMIT = 4,         /* a property exceeds the limits given at create          */
    PSK_SOFT_ERR_UNSUPPORTED = 5,   /* samplesPerBaud == 0 or phaseAvg == 0 (undefined in the
                                       reference: cpp/psk_soft.cpp:441,454 and :54-55,70)     */
    PSK_SOFT_ERR_CAPACITY = 6       /* an output buffer is too small                          */
} psk_soft_status;

/* serviceFunction() return codes, reference cpp/psk_soft.cpp:351,362,617 */
enum { PSK_SOFT_NOOP = 0, PSK_SOFT_NORMAL = 1 };

/* device == PSK_SOFT_DEVICE_NONE creates a control-plane-only handle: property,
 * flag, SRI and output-count logic run (they are host-side), no data is touched. */
#define PSK_SOFT_DEVICE_NONE (-1)

/* The six properties, reference psk_soft.prf.xml:23-60 / cpp/psk_soft_base.h:45-56.
 * Same names, types and defaults (cpp/psk_soft_base.cpp:96-148). */
typedef struct psk_soft_props {
    uint16_t samplesPerBaud;       /* ushort, default 10  */
    uint16_t constelationSize;     /* ushort, default 4   */
    uint32_t numAvg;               /* ulong,  default 100 */
    uint16_t phaseAvg;             /* ushort, default 50  */
    uint8_t differentialDecoding;  /* bool,   default 0   */
    uint8_t resetState;            /* bool,   default 0; self-clearing (cpp/psk_soft.cpp:365-372) */
} psk_soft_props_t;

/* Upper bounds that size the per-channel state in HBM. */
typedef struct psk_soft_limits {
    uint32_t max_window_samples;   /* >= samplesPerBaud*numAvg of every channel (the `samples` deque) */
    uint32_t max_phase_avg;        /* >= phaseAvg of every channel (LinearFit::yvals)                 */
    uint32_t max_packet_complex;   /* >= complex samples of one packet of one channel (host-buffer path), either format */
} psk_soft_limits_t;

/* Sample format of a packet (psk_soft_packet_t::format), per packet: one call may mix formats and a channel may change
 * format from one call to the next (the carried window holds converted samples).
 *   PSK_SOFT_FORMAT_CF32  interleaved float32 I,Q (bulkio::InFloatPort); `data` 8-byte aligned.
 *   PSK_SOFT_FORMAT_CS16  interleaved int16 I,Q (sc16, bulkio::InShortPort); `data` 4-byte aligned.  Every call gives
 *                         bit for bit what the CF32 packet of the values (float)v gives (the cast is exact); the
 *                         library converts on the GPU, the packet crosses the link and sits in memory at half the size.
 *   PSK_SOFT_FORMAT_CS8   interleaved int8 I,Q (sc8, bulkio::InCharPort dataChar); `data` 2-byte aligned (whole complex
 *                         samples).  Bit for bit what the CF32 packet -- and the CS16 packet -- of the values (float)v
 *                         gives; a quarter of the float packet's bytes.
 *   PSK_SOFT_FORMAT_CF16  interleaved IEEE binary16 I,Q, little-endian, I first (cf16; torch.complex32 is this layout);
 *                         `data` 4-byte aligned (whole complex samples).  Bit for bit what the CF32 packet of the widened
 *                         values gives: binary16 -> binary32 is exact for every finite value and the infinities, half
 *                         subnormals become normal floats (never flushed), a quiet NaN keeps its sign and its payload
 *                         shifted left by 13 bits.  Signalling-NaN encodings (exponent 31, mantissa non-zero, bit 9 clear)
 *                         are outside that contract: the result is that of some NaN.  Half the float packet's bytes.
 * Any other value (2, 5, 6, 7 among them) is refused with PSK_SOFT_ERR_INVALID_ARG before anything is enqueued.  (ABI version 2 before this
 * field had a name called it `reserved` and ignored it: callers that left garbage there must zero it.) */
enum { PSK_SOFT_FORMAT_CF32 = 0, PSK_SOFT_FORMAT_CS16 = 1, PSK_SOFT_FORMAT_CS8 = 3, PSK_SOFT_FORMAT_CF16 = 4 };

/* One bulkio::InFloatPort (or InShortPort, InCharPort) ::dataTransfer as serviceFunction() reads it
 * (reference cpp/psk_soft.cpp:349-359, 394, 428). */
typedef struct psk_soft_packet {
    const float *data;          /* dataBuffer: interleaved I,Q (device or host pointer, per entry point); for
                                   PSK_SOFT_FORMAT_CS16 it points at int16 elements, for PSK_SOFT_FORMAT_CS8 at int8
                                   elements, for PSK_SOFT_FORMAT_CF16 at binary16 elements (cast the pointer)   */
    uint64_t n_floats;          /* dataBuffer.size(): ELEMENTS of the packet's format (floats, int16s, int8s, halves); the
                                   packet holds n_floats / 2 complex samples, an odd last element is ignored   */
    double sri_xdelta;          /* SRI.xdelta                                                             */
    int32_t sri_mode;           /* SRI.mode; anything but 1 is dropped with a warning (:359-363)          */
    uint8_t sriChanged;
    uint8_t inputQueueFlushed;  /* forces resetState (:353-357)                                           */
    uint8_t present;            /* 0 = getPacket() returned NULL for this channel: NOOP (:350-352)        */
    uint8_t format;             /* PSK_SOFT_FORMAT_CF32 / _CS16 / _CS8 / _CF16 (checked on present packets)  */
} psk_soft_packet_t;

/* Where one channel's four output streams go, and what the call produced.
 * Layout advice for the device-pointer path: start every channel's row of every stream on a
 * 128-byte boundary (e.g. a row capacity that is a multiple of 64 symbols).  The kernels store
 * whole cache lines per wave; rows that straddle lines were measured 6 % slower end to end.
 * Pointer fields are inputs; the rest is filled in before the call returns
 * (output sizes depend only on packet sizes and properties, so they are exact
 * even on the asynchronous device-pointer path). */
typedef struct psk_soft_output {
    float *soft;                /* softDecision_dataFloat_out payload: re,im per symbol */
    int16_t *bits;              /* bits_dataShort_out: log2(M) shorts per symbol        */
    float *phase;               /* phase_dataFloat_out: one per symbol                  */
    int16_t *sampleIndex;       /* sampleIndex_dataShort_out: one per symbol            */
    uint64_t cap_symbols;       /* capacity of the buffers above, in symbols: soft holds 2 * cap floats, phase cap, bits
                                   cap * log2(M) shorts, sampleIndex cap.  One rule on every entry: a call that emits more
                                   symbols into the channel than cap_symbols is refused with PSK_SOFT_ERR_CAPACITY, before
                                   anything is committed or enqueued, when ANY of the four pointers is non-null (bits or
                                   sampleIndex alone count); exactly n_symbols is enough; all four null needs no room (0) */
    /* results */
    int32_t ret;                /* PSK_SOFT_NOOP / PSK_SOFT_NORMAL                      */
    uint64_t n_symbols;         /* symbols emitted: soft has 2*n, phase n                */
    uint64_t n_bits;            /* shorts written to bits (n * bitsPerBaud)             */
    uint64_t n_sampleIndex;     /* n, or 0 when samplesPerBaud == 1 (:459-469)          */
    int32_t sri_pushed;         /* 1: the host must pushSRI on soft/phase/bits (:393-405) */
    double sri_soft_xdelta;     /* xdelta for the soft and phase SRIs (:399)            */
    double sri_bits_xdelta;     /* xdelta for the bits SRI (:403)                       */
    int32_t n_warn;             /* LOG_WARN count (:355,361,566)                        */
} psk_soft_output_t;

typedef struct psk_soft_handle psk_soft_handle_t;

/* Runtime statistics of the last psk_soft_process_* call (read after psk_soft_synchronize).  A control-
 * plane-only handle (PSK_SOFT_DEVICE_NONE) fills in channels_fast / channels_sequential as PLANNED. */
typedef struct psk_soft_stats {
    uint64_t channels_fast;       /* channels handled by a wave-scan kernel                        */
    uint64_t channels_exact_timing; /* of those: calls whose timing screening refused (near-ties) and
                                       that the exact-timing wave-scan kernel redid                */
    uint64_t channels_sequential; /* channels handled by the reference-order kernel (planned)      */
    uint64_t channels_guard;      /* of those: sent there at run time by the exactness guard       */
    uint64_t unwrap_extra_passes; /* extra unwrap fixed-point passes summed over all 128-symbol blocks */
    uint64_t unwrap_blocks;       /* 128-symbol blocks processed by the wave-scan kernel           */
    uint64_t timing_exact_blocks; /* of those: blocks whose timing argmax needed the exact double pass
                                     (in the screened kernel, numAvg <= 128, or in the exact kernel) */
    uint64_t fit_chain_blocks;    /* of those: blocks whose LinearFit sums were redone in the reference's
                                     order of additions by the lane-after-lane chain (the wave-parallel
                                     candidates did not verify: sums crossing a binade or zero)          */
    uint64_t channels_tiled;      /* of channels_fast: calls carried by the time-tiled kernels (few channels,
                                     long packets: the call is cut along time, see PSK_SOFT_OPT_TIME_TILED) */
    uint64_t channels_parallel_fit; /* of channels_tiled: calls whose feedback unwrap and fit were guessed and
                                     verified in parallel along time instead of walked block by block   */
    uint64_t channels_parallel_fit_second_round; /* of channels_parallel_fit: on the second guess of the unwrap counts
                                     (the first, by consecutive raw phases, was wrong somewhere: a noisy stream)      */
    uint64_t parallel_fit_refusals; /* why tiled calls that tried did not: bit 0 a ySum that rounds, bit 1 an xySum
                                     certificate, bit 2 an unwrap count the guess got wrong (OR over the channels) */
} psk_soft_stats_t;

uint32_t psk_soft_abi_version(void);
const char *psk_soft_last_error(void);            /* thread-local text of the last failure */

/* lifetime -- replaces the psk_soft_i constructor (cpp/psk_soft.cpp:187-213): every
 * channel starts with the default properties, empty history and all three reset flags set. */
psk_soft_status psk_soft_create(int device, uint32_t n_channels, const psk_soft_limits_t *limits,
                                psk_soft_handle_t **out);
psk_soft_status psk_soft_destroy(psk_soft_handle_t *h);

/* configure() of channels [ch0, ch0+nch): stores the properties and runs the change
 * listeners the component registers (cpp/psk_soft.cpp:210-212, 638-651) for every
 * property whose value differs from the stored one.  Takes effect at the next process call
 * (the reference snapshots its properties at the top of serviceFunction, :374-378).
 * Every samplesPerBaud the ushort property holds (1 .. 65535) is accepted; PSK_SOFT_ERR_LIMIT only when
 * samplesPerBaud*numAvg exceeds max_window_samples or phaseAvg max_phase_avg. */
psk_soft_status psk_soft_configure(psk_soft_handle_t *h, uint32_t ch0, uint32_t nch,
                                   const psk_soft_props_t *props /* [nch] */);
psk_soft_status psk_soft_query(const psk_soft_handle_t *h, uint32_t ch, psk_soft_props_t *props);
/* run one listener unconditionally: 0 samplesPerBaudChanged, 1 constelationSizeChanged, 2 phaseAvgChanged */
psk_soft_status psk_soft_fire_listener(psk_soft_handle_t *h, uint32_t ch, int which);

/* symbols one call can emit for a packet of n_complex samples: (n_complex + samplesPerBaud-1)/samplesPerBaud
 * bounds the reference's reserve() at cpp/psk_soft.cpp:434 */
uint64_t psk_soft_output_capacity(const psk_soft_handle_t *h, uint32_t ch, uint64_t n_complex);

/* One serviceFunction() body for channels [ch0, ch0+nch), one packet each.
 * _device: packet data and output buffers are DEVICE pointers; kernels are enqueued on
 *          `stream` (a hipStream_t, NULL = the handle's own stream) and the call returns
 *          without waiting; counts/SRI fields of `outs` are already final.
 * _host:   packet data and output buffers are HOST pointers; the library stages them
 *          through HBM and returns when the outputs are in place. */
psk_soft_status psk_soft_process_device(psk_soft_handle_t *h, uint32_t ch0, uint32_t nch,
                                        const psk_soft_packet_t *pkts /* [nch] */,
                                        psk_soft_output_t *outs /* [nch] */, void *stream);
psk_soft_status psk_soft_process_host(psk_soft_handle_t *h, uint32_t ch0, uint32_t nch,
                                      const psk_soft_packet_t *pkts, psk_soft_output_t *outs);
psk_soft_status psk_soft_synchronize(psk_soft_handle_t *h);

/* psk_soft_process_device for packets whose samples are not contiguous: channelizer output, written frame by frame
 * ([frame][channel]: for each time step one sample of every channel), handed over as it lies.
 *   sample_stride[i]  distance between consecutive complex samples of packet i, counted in complex samples of that packet's
 *                     format: sample k is the adjacent I,Q pair at element offset 2*k*sample_stride[i] from `data`.  For
 *                     channel c of a matrix `width` channels wide: data = base + 2*c elements, sample_stride = width.
 *   n_floats          as ever the packet's OWN elements (2 per sample, an odd last element ignored).  The library reads exactly
 *                     those n_floats / 2 pairs, nothing between or behind them, and never writes to the caller's buffer.
 * A stride of 1 -- or sample_stride == NULL, for the whole call -- is psk_soft_process_device: the same code path, no gather.
 * One call may mix strided and contiguous packets, and formats.  `data` is aligned as the format asks (8 / 4 / 2 bytes: whole
 * samples); the caller's buffer lives as long as for psk_soft_process_device (until the call's work on `stream` is done).
 * Refused with PSK_SOFT_ERR_INVALID_ARG before anything is planned, committed or enqueued: a stride of 0 on a present packet,
 * and an extent stride x bytes-per-sample x samples that does not fit 64 bits.
 * Results: every output stream, count, SRI field, warning count, statistic and quality record is bit for bit what
 * psk_soft_process_device gives for the contiguous packet holding the same samples, under every schedule and option.
 *
 * How: the strided packets are first gathered, on `stream`, into contiguous rows of a gather scratch the handle owns, in their
 * own format (2 / 4 / 8 bytes a sample; rows 128-byte aligned), and the ordinary call runs on the rows.  Runs of at least 8
 * consecutive packets of one format and stride whose `data` pointers lie exactly one sample apart -- adjacent columns of one
 * matrix, lengths may differ -- take a tiled transpose that reads whole runs of bytes of every frame; any other strided packet
 * is gathered sample by sample, each load a memory line of its own: correct and slow.  Keep a matrix's channels consecutive in
 * the call.
 * The scratch: one buffer per calling stream (four in all; a fifth stream takes over the one used longest ago, behind the
 * event that ends its last call), grown to 1.25 x the largest call seen and never shrunk; growing is the one place that waits
 * for the device.  With PSK_SOFT_OPT_DEFERRED_JOIN a class of an earlier call may still be reading its rows on a side stream
 * when the next strided call arrives: that call JOINS the side streams into `stream` before it gathers (as psk_soft_join
 * would), so rows are never overwritten while in use; calls without strided packets keep the deferred join as it is.
 * A control-plane-only handle checks the strides, then plans and counts like psk_soft_process_device.
 * There is no host-pointer counterpart: a host with pageable frame-major data gathers while it stages. */
psk_soft_status psk_soft_process_device_strided(psk_soft_handle_t *h, uint32_t ch0, uint32_t nch,
                                                const psk_soft_packet_t *pkts /* [nch] */,
                                                const uint64_t *sample_stride /* [nch], or NULL */,
                                                psk_soft_output_t *outs /* [nch] */, void *stream);

/* ---- tuned packets: a frequency shift per packet, applied on the GPU in front of the demodulator ------------------------------
 * A channelizer delivers each signal wherever it falls inside its bin, and the M-th-power phase tracker of serviceFunction()
 * (reference cpp/psk_soft.cpp:474-482) follows only a small carrier offset: lock (psk_soft_quality_derive) falls from 0.98 at
 * 0.05 cycles per symbol to 0.1 at 0.10 for QPSK, and is gone at 0.05 for 8-PSK.  A tuned packet is multiplied by a numerically
 * controlled oscillator before anything else looks at it.
 *
 * The definition (host and device alike).  phase and step are in turns x 2^64; all arithmetic on them is mod 2^64.  Sample k
 * (k = 0 .. n_floats / 2 - 1) of the packet is
 *   - converted to float exactly, as its format defines (above);
 *   - multiplied by the phasor W(p_k), p_k = phase + k * step, taken from two tables of 1024 entries with
 *       h = p_k >> 54,  l = (p_k >> 44) & 1023          (the top 20 bits; the phase word is truncated, as in any DDS)
 *       C[h] = (cosf(a), sinf(a)),  a = (float)((double)h * 0x1.921fb54442d18p-8)     (pi / 512)
 *       F[l] = (cosf(b), sinf(b)),  b = (float)((double)l * 0x1.921fb54442d18p-18)    (pi / 2^19)
 *     cosf and sinf being glibc 2.35's (the library carries them: they do not depend on the libm it runs with),
 *       W = (Cr*Fr - Ci*Fi,  Cr*Fi + Ci*Fr)
 *       y = (xr*Wr - xi*Wi,  xr*Wi + xi*Wr)
 *     every operation float32, rounded once, no fused multiply-add, denormals kept.
 * W(0) = (1, 0) exactly; | |W| - 1 | <= 1.4e-7; the angle of W is that of the truncated phase to 3.3e-7 rad, on top of the
 * quantum of 6e-6 rad (2 pi / 2^20).
 * The result of the call is bit for bit what the contiguous PSK_SOFT_FORMAT_CF32 packet holding the y values gives: all four
 * streams, counts, SRI fields, warnings, statistics and quality records, under every schedule and option.  That contract covers
 * samples whose y is finite; with a non-finite sample or product the formula above is still what runs, and which NaN comes out
 * is unspecified.  A packet whose tune is {0, 0} is not tuned at all: it takes exactly the path it takes without `tune`, the
 * in-place builds of the integer formats included, and keeps the sign of -0.
 * The oscillator's state belongs to the caller: the library keeps nothing between calls (state blobs are unchanged); the phase
 * word of a stream's next packet is psk_soft_tune_advance(). */
typedef struct psk_soft_tune {
    uint64_t phase;   /* phase word of the packet's sample 0  */
    uint64_t step;    /* phase increment per complex sample   */
} psk_soft_tune_t;

/* psk_soft_process_device_strided with tune[i] applied to packet i.  tune == NULL is psk_soft_process_device_strided: the same
 * code path.  Strides are checked and refused as there; every phase / step value is valid.  One call may mix tuned and untuned
 * packets, strides and formats.
 * How: one more launch on `stream` behind the gathers writes every tuned packet, shifted, as a float2 row (8 bytes a sample,
 * whatever the packet's format; 128-byte aligned) of the gather scratch, and the ordinary call runs on those rows as on CF32
 * packets.  A tuned strided packet in a run the tiled transpose takes (at least 8 adjacent columns, see above) is first gathered
 * into a row of its own format and tuned from there; any other tuned packet, contiguous or strided, is read where it lies.
 * Scratch, descriptor slots, events and the deferred-join rule are those of psk_soft_process_device_strided.
 * A control-plane-only handle checks, then plans and counts like psk_soft_process_device.  No host-pointer counterpart. */
psk_soft_status psk_soft_process_device_tuned(psk_soft_handle_t *h, uint32_t ch0, uint32_t nch,
                                              const psk_soft_packet_t *pkts /* [nch] */,
                                              const uint64_t *sample_stride /* [nch], or NULL */,
                                              const psk_soft_tune_t *tune /* [nch], or NULL */,
                                              psk_soft_output_t *outs /* [nch] */, void *stream);

/* Host only, pure.
 * psk_soft_tune_step: the step word of a shift by `cycles_per_sample` (negative = downwards): r = f - floor(f), the result
 *   (uint64_t)(r * 2^64), truncated, mod 2^64; 0 for a non-finite f.  To take a channel's carrier offset of f cycles per
 *   sample OUT, tune with psk_soft_tune_step(-f).
 * psk_soft_tune_advance: phase + step * n_complex (mod 2^64): the phase word of the next packet of a continuous stream.
 * psk_soft_tune_apply: the definition above for n_complex CF32 samples, in to out (in == out allowed). */
uint64_t psk_soft_tune_step(double cycles_per_sample);
uint64_t psk_soft_tune_advance(uint64_t phase, uint64_t step, uint64_t n_complex);
psk_soft_status psk_soft_tune_apply(const psk_soft_tune_t *tune, const float *in, uint64_t n_complex, float *out);

/* ---- resampled packets: a fractional resampler per packet, applied on the GPU in front of the demodulator --------------------
 * samplesPerBaud is an integer (the reference's ushort property): the per-symbol loop of serviceFunction() steps a whole number
 * of samples per symbol.  A channelizer hands every bin the same sample rate, and a signal's symbol rate almost never divides
 * it; QPSK at 8.37 samples a symbol demodulated with samplesPerBaud 8 is lost, not degraded.  A resampled packet is brought to
 * an integer number of samples per symbol before anything else looks at it: `step` input samples per output sample.
 *
 * The definition (host and device alike).  pos and step are in input samples x 2^32.
 *   Input samples.  Sample k of the packet is converted to float exactly, as its format defines; if the packet is also tuned it
 *     is multiplied by the NCO exactly as "tuned packets" (above) defines, k counted from the packet's sample 0.  Call the result
 *     s[k], k = 0 .. n-1, n = n_floats / 2.  s[-3], s[-2], s[-1] are the channel's HISTORY: the last three s values in front of
 *     this packet, already tuned, oldest first; zeros with PSK_SOFT_RS_RESTART.
 *   Output instants.  t_m = pos + m * step for m = 0, 1, .. while t_m < n * 2^32; n_out is the count of those m.
 *   Per output:  i = t_m >> 32,  mu = (float)((t_m & 0xffffffff) >> 8) * 0x1p-24f  (the conversion is exact), then
 *       a = mu, b = mu - 1, c = mu - 2, d = mu + 1
 *       w0 = ((a*b)*c) * (float)(-1.0/6.0)     w1 = ((d*b)*c) * 0.5f
 *       w2 = ((d*a)*c) * -0.5f                 w3 = ((d*a)*b) * (float)(1.0/6.0)
 *       y  = ((w0*s[i-3] + w1*s[i-2]) + w2*s[i-1]) + w3*s[i]                  (re and im separately)
 *     every operation float32, rounded once, no fused multiply-add, denormals kept.
 *   This is the cubic Lagrange polynomial through four consecutive samples, evaluated between s[i-2] and s[i-1]: a pure delay
 *   of TWO input samples, which is what lets a packet be resampled without its successor.  At mu = 0 the result is s[i-2]:
 *   step = 2^32, pos = 0 returns the stream delayed by two samples, bit for bit (the weights are -0, 1, +0, -0: only the sign of
 *   a zero sample can change, with its neighbours' signs).
 *   After the packet.  The new history is the last three of (old history || s[0 .. n-1]); the next packet's position is
 *     pos + n_out * step - n * 2^32, always below step (psk_soft_resample_advance).
 * The result of the call is bit for bit what the contiguous PSK_SOFT_FORMAT_CF32 packet holding y[0 .. n_out-1] gives, with
 * sri_xdelta * ((double)step * 0x1p-32) as its sri_xdelta: all four streams, counts, SRI fields, warnings, statistics and quality
 * records, under every schedule and option.  That contract covers finite y; with non-finite samples the formula above is still
 * what runs, and which NaN comes out is unspecified.
 * THERE IS NO ANTI-ALIAS FILTER.  The signal must be oversampled (as a signal at several samples per symbol is) and step must
 * stay near 1 -- the use case is a sample rate a few percent to a few tens of percent off an integer number of samples per
 * symbol.  Size the output rows with psk_soft_output_capacity(h, ch, n_out), n_out from psk_soft_resample_count(). */
enum { PSK_SOFT_RS_RESTART = 1 };
typedef struct psk_soft_resample {
    uint64_t pos;     /* position of the packet's first output sample, in input samples x 2^32, counted from the packet's sample 0 */
    uint64_t step;    /* input samples per output sample x 2^32; 0 = this packet is not resampled (pos, flags ignored)            */
    uint32_t flags;   /* PSK_SOFT_RS_RESTART: the history in front of the packet is three zero samples                            */
    uint32_t pad;     /* zero */
} psk_soft_resample_t;   /* 24 bytes */

/* psk_soft_process_device_tuned with resample[i] applied to packet i.  resample == NULL is psk_soft_process_device_tuned: the
 * same code path; a packet with step == 0 takes exactly the path it takes there, the in-place builds of the integer formats
 * included, and costs no extra launch.  A packet that is absent, has sri_mode != 1 or has no samples is left to the ordinary
 * call (a NOOP or a warning, as before) and the channel's history does not change.  One call may mix resampled and
 * not-resampled packets, tuned or not, strides and formats.
 * Refused with PSK_SOFT_ERR_INVALID_ARG before anything is planned, committed or enqueued, on a present packet with step != 0:
 * a step outside [2^31, 2^33], pos > 2^33, n_floats / 2 >= 2^30, a non-zero pad, unknown flag bits; and whatever
 * psk_soft_process_device_strided refuses.
 * How: every resampled packet gets a float2 row of n_out samples (128-byte aligned) in the gather scratch, and ONE more launch
 * on `stream` behind the gathers writes the rows; the ordinary call runs on them as on CF32 packets of n_out samples with the
 * scaled sri_xdelta.  A resampled packet that is also tuned is tuned inside that launch (no tune row, no second pass); tuned-only
 * packets of the call still go through the tune pass.  A strided packet in a run the tiled transpose takes (at least 8 adjacent
 * columns) is read from its gathered row, any other where it lies.  Scratch, descriptor slots, events and the deferred-join
 * rule are those of psk_soft_process_device_strided.
 * History: device memory the handle owns, two slots of three float2 per channel, allocated at the first resampled call.  A
 * launch reads the channel's current slot and writes the other; the slots change roles only when the whole call returned
 * PSK_SOFT_OK, so a refused call (PSK_SOFT_ERR_CAPACITY, PSK_SOFT_ERR_LIMIT, ..) changes nothing a later call can see.  The
 * history is not part of the state blob (psk_soft_state_bytes is unchanged): checkpoint it with the two calls below.
 * A control-plane-only handle checks the arguments, then plans and counts on n_out and the scaled sri_xdelta; its history stays
 * zero.  No host-pointer counterpart; psk_soft_acquire_device does not resample. */
psk_soft_status psk_soft_process_device_resampled(psk_soft_handle_t *h, uint32_t ch0, uint32_t nch,
                                                  const psk_soft_packet_t *pkts /* [nch] */,
                                                  const uint64_t *sample_stride /* [nch], or NULL */,
                                                  const psk_soft_tune_t *tune /* [nch], or NULL */,
                                                  const psk_soft_resample_t *resample /* [nch], or NULL */,
                                                  psk_soft_output_t *outs /* [nch] */, void *stream);
/* the history of channel ch, three (re, im) pairs, oldest first.  _get waits for the last resampled call's pass, as
 * psk_soft_get_quality waits for its own; _set replaces it (continue a checkpointed stream, tests). */
psk_soft_status psk_soft_resample_get_history(psk_soft_handle_t *h, uint32_t ch, float *out /* [6] */);
psk_soft_status psk_soft_resample_set_history(psk_soft_handle_t *h, uint32_t ch, const float *in /* [6] */);

/* Host only, pure.
 * psk_soft_resample_step: the step word of `in_per_out` input samples per output sample, (uint64_t)(r * 2^32), truncated; 0 for
 *   a non-finite value or one outside [0.5, 2].  For a signal at sps samples per symbol and samplesPerBaud S: sps / S.
 * psk_soft_resample_count: n_out of a packet of n_complex samples (step == 0: n_complex, the packet goes as it is).
 * psk_soft_resample_advance: pos of the stream's next packet (step == 0: pos).
 * psk_soft_resample_apply: the definition above for n_complex untuned CF32 samples.  hist_in NULL or PSK_SOFT_RS_RESTART: a
 *   history of zeros; hist_out (may be NULL) receives the history behind the packet; `out` holds psk_soft_resample_count()
 *   samples; `in` and `out` must not overlap.  Refuses what the entry refuses, and step == 0. */
uint64_t psk_soft_resample_step(double in_per_out);
uint64_t psk_soft_resample_count(const psk_soft_resample_t *rs, uint64_t n_complex);
uint64_t psk_soft_resample_advance(const psk_soft_resample_t *rs, uint64_t n_complex);
psk_soft_status psk_soft_resample_apply(const psk_soft_resample_t *rs, const float *hist_in /* [6] or NULL */, const float *in,
                                        uint64_t n_complex, float *out, float *hist_out /* [6] or NULL */);
uint32_t psk_soft_resample_piece(void);     /* outputs of one workgroup's piece of the device's pass (tests: the lengths at its edges) */

/* ---- filtered packets: a decimating FIR (a matched filter) per packet, applied on the GPU in front of the demodulator ---------
 * The demodulator has no integrate-and-dump: its timing stage integrates ENERGY per intra-symbol phase and then picks ONE sample
 * per symbol, so at samplesPerBaud 8 seven of eight samples contribute nothing to a decision.  A matched filter in front puts
 * the whole symbol's energy into the sample the timing stage picks (QPSK at 8 samples a symbol, noise sigma 0.5 a component:
 * 1688 of 5700 differential decisions wrong without, 9 behind eight taps of 1/8), and it is the anti-alias filter the resampler
 * does not have.  Filters are real-tap FIRs the handle keeps in PSK_SOFT_FIR_SLOTS numbered slots (psk_soft_fir_define).
 *
 * The definition (host and device alike).
 *   Input samples.  Sample k of the packet is converted to float exactly, as its format defines; if the packet is also tuned it
 *     is multiplied by the NCO exactly as "tuned packets" (above) defines.  Call the result s[k], k = 0 .. n-1, n = n_floats / 2.
 *   History.  s[-127] .. s[-1] are the channel's HISTORY: the last PSK_SOFT_FIR_MAX_TAPS - 1 values of s in front of this packet,
 *     already tuned, oldest first; zeros with PSK_SOFT_FIR_RESTART.  It always holds 127 samples, whatever the filter's length:
 *     a stream may change its filter between packets and the result is still defined.
 *   Outputs.  m = 0, 1, .. while i_m = pos + m * decim < n; n_out is their count: 0 if pos >= n, else (n - pos + decim - 1) / decim.
 *   Per output, with the taps h[0 .. T-1], re and im separately:
 *       acc = h[0] * s[i]
 *       acc = acc + h[j] * s[i-j]     for j = 1 .. T-1, in that order
 *     every operation float32, rounded once, no fused multiply-add, denormals kept.
 *   After the packet.  The new history is the last 127 of (old history || s[0 .. n-1]); the next packet's pos is
 *     pos + n_out * decim - n, always below decim (psk_soft_fir_advance).  A packet with samples but no outputs (pos >= n) still
 *     moves the history.
 * The result of the call is bit for bit what psk_soft_process_device_resampled gives for the contiguous PSK_SOFT_FORMAT_CF32
 * packet holding y[0 .. n_out-1], untuned, with the same resample[i] and sri_xdelta * (double)decim as its sri_xdelta (which the
 * resampler then scales as it always does): all four streams, counts, SRI fields, warnings, statistics and quality records, under
 * every schedule and option.  That contract covers finite y; with non-finite samples or taps the formula above is still what
 * runs, and which NaN comes out is unspecified.
 * Two identities follow.  The taps {1.0f} with decim 1 give the unfiltered call bit for bit for finite samples, the sign of a
 * zero included (y = 1 * s).  The taps {0, 0, 1} give the stream delayed by two samples, except for the sign of a zero sample
 * (0*a + 0*b + (-0) is +0).
 * The filter's group delay ((T-1)/2 input samples for symmetric taps) is the caller's bookkeeping: nothing in the SRI moves.
 * THE DECIMATION PHASE MATTERS: of the decim possible values of pos one keeps the matched filter's peak ("A
 * matched filter in front of the demodulator").  Size the output rows with psk_soft_output_capacity(h, ch, n_out), n_out from
 * psk_soft_fir_count() (and psk_soft_resample_count() on that, if the packet is resampled as well). */
#define PSK_SOFT_FIR_MAX_TAPS 128
#define PSK_SOFT_FIR_SLOTS    64
#define PSK_SOFT_FIR_MAX_DECIM 16
enum { PSK_SOFT_FIR_RESTART = 1 };
typedef struct psk_soft_fir {
    uint32_t filter;  /* 1 + slot; 0 = this packet is not filtered (decim, pos, flags ignored) */
    uint32_t decim;   /* D: 1 .. 16, input samples per output sample                           */
    uint32_t pos;     /* index, in the packet, of the newest input of the first output; < decim */
    uint32_t flags;   /* PSK_SOFT_FIR_RESTART: the history in front of the packet is zeros      */
} psk_soft_fir_t;     /* 16 bytes */

/* The taps of slot `slot` (0 .. PSK_SOFT_FIR_SLOTS - 1): 1 .. PSK_SOFT_FIR_MAX_TAPS floats, copied into device memory the
 * handle owns (SLOTS x MAX_TAPS floats, allocated at the first define).  Waits first for the last filter launch of the handle, so
 * redefining a slot never races a launch that reads it -- the one place besides scratch growth that waits.  A control-plane-only
 * handle records n_taps only.  PSK_SOFT_ERR_INVALID_ARG: null, slot >= 64, n_taps 0 or above 128. */
psk_soft_status psk_soft_fir_define(psk_soft_handle_t *h, uint32_t slot, const float *taps, uint32_t n_taps);

/* psk_soft_process_device_resampled with fir[i] applied to packet i, behind the frequency shift and in front of the resampler.
 * fir == NULL is psk_soft_process_device_resampled: the same code path; a packet with filter == 0 takes exactly the path it
 * takes there.  A packet that is absent, has sri_mode != 1 or has no samples is left to the ordinary call and the channel's
 * history does not change.  One call may mix packets that are filtered, tuned, resampled and strided in every combination, and
 * may mix formats.
 * Refused with PSK_SOFT_ERR_INVALID_ARG before anything is planned, committed or enqueued, on a present packet with
 * filter != 0: a slot >= 64 or never defined, decim 0 or above 16, pos >= decim, unknown flag bits, n_floats / 2 >= 2^30; and
 * whatever psk_soft_process_device_resampled refuses.
 * How: every filtered packet gets a float2 row of n_out samples (128-byte aligned) in the gather scratch, and ONE more launch on
 * `stream`, behind the gathers and the tune pass and in front of the resample pass, writes the rows.  A filtered packet that is
 * also tuned is tuned inside that launch (no tune row).  A packet both filtered and resampled is resampled from its filter row
 * (CF32, n_out samples, not tuned) into a row of its own: it pays two passes.  A strided packet in a run the tiled transpose
 * takes (at least 8 adjacent columns) is read from its gathered row, any other where it lies.  The ordinary call then runs on CF32
 * packets of the final count with the scaled sri_xdelta.  Scratch, descriptor slots, events and the deferred-join rule are those
 * of psk_soft_process_device_strided.
 * History: device memory the handle owns, two slots of 127 float2 (1 KiB each) per channel, allocated at the first filtered
 * call.  A launch reads the channel's current slot and writes the other; the slots change roles only when the whole call
 * returned PSK_SOFT_OK, so a refused call (PSK_SOFT_ERR_CAPACITY, PSK_SOFT_ERR_LIMIT, ..) changes nothing a later call can see.
 * The history is not part of the state blob: checkpoint it with the two calls below.
 * A control-plane-only handle checks the arguments, then plans and counts on the final count and sri_xdelta; its history stays
 * zero.  No host-pointer counterpart; psk_soft_acquire_device does not filter. */
psk_soft_status psk_soft_process_device_filtered(psk_soft_handle_t *h, uint32_t ch0, uint32_t nch,
                                                 const psk_soft_packet_t *pkts /* [nch] */,
                                                 const uint64_t *sample_stride /* [nch], or NULL */,
                                                 const psk_soft_tune_t *tune /* [nch], or NULL */,
                                                 const psk_soft_fir_t *fir /* [nch], or NULL */,
                                                 const psk_soft_resample_t *resample /* [nch], or NULL */,
                                                 psk_soft_output_t *outs /* [nch] */, void *stream);
/* the history of channel ch, 127 (re, im) pairs, oldest first.  _get waits for the last filter pass; _set replaces it. */
psk_soft_status psk_soft_fir_get_history(psk_soft_handle_t *h, uint32_t ch, float *out /* [254] */);
psk_soft_status psk_soft_fir_set_history(psk_soft_handle_t *h, uint32_t ch, const float *in /* [254] */);

/* Host only, pure.
 * psk_soft_fir_count: n_out of a packet of n_complex samples (filter == 0: n_complex, the packet goes as it is).
 * psk_soft_fir_advance: pos of the stream's next packet (filter == 0: pos).
 * psk_soft_fir_apply: the definition above for n_complex untuned CF32 samples and the given taps (f->filter is not looked at).
 *   hist_in NULL or PSK_SOFT_FIR_RESTART: a history of zeros; hist_out (may be NULL) receives the history behind the packet;
 *   `out` holds psk_soft_fir_count() samples; `in` and `out` must not overlap.  Refuses what the entry refuses.
 * psk_soft_fir_piece: outputs of one workgroup's piece of the device's pass at that decim (tests: the lengths at its edges). */
uint64_t psk_soft_fir_count(const psk_soft_fir_t *f, uint64_t n_complex);
uint32_t psk_soft_fir_advance(const psk_soft_fir_t *f, uint64_t n_complex);
psk_soft_status psk_soft_fir_apply(const psk_soft_fir_t *f, const float *taps, uint32_t n_taps, const float *hist_in /* [254] or NULL */,
                                   const float *in, uint64_t n_complex, float *out, float *hist_out /* [254] or NULL */);
uint32_t psk_soft_fir_piece(uint32_t decim);

/* PSK_SOFT_OPT_DEFERRED_JOIN: make `stream` (a hipStream_t; NULL = the handle's own) wait for everything the calls made so
 * far have put on the handle's side streams -- the point in stream order behind which their results may be used.  A no-op
 * without pending deferred calls.  (There is no counterpart in the reference: its serviceFunction() is synchronous.) */
psk_soft_status psk_soft_join(psk_soft_handle_t *h, void *stream);
psk_soft_status psk_soft_get_stats(psk_soft_handle_t *h, psk_soft_stats_t *stats);
/* the same, one record per channel of [ch0, ch0+nch) (stats[nch]) */
psk_soft_status psk_soft_get_channel_stats(psk_soft_handle_t *h, uint32_t ch0, uint32_t nch, psk_soft_stats_t *stats);

/* Options of a handle (all default 0 = the reference's behaviour, quirks included).
 * PSK_SOFT_OPT_QPSK_SIGN_BITMAP: 1 = QPSK bits by the signs of the de-rotated symbol, as the
 *   constellation diagram at reference cpp/psk_soft.cpp:516-521 describes (A 00, B 01, C 10, D 11,
 *   least significant bit first), instead of the float->bool conversions of :523-526 that make
 *   every QPSK bit 0.  Opt-in; takes effect at the next process call. */
enum {
    PSK_SOFT_OPT_QPSK_SIGN_BITMAP = 1,
    /* 1 (default): a batch that mixes window classes (samplesPerBaud, numAvg <= 128 / 256 / 512 / 1024) launches its
     * classes side by side on streams of the handle, forked off and joined back into the caller's stream; 0: one
     * after the other on the caller's stream.  No effect on results. */
    PSK_SOFT_OPT_CONCURRENT_CLASSES = 2,
    /* Calls of few channels and many symbols are cut along time (tiles of a few hundred symbols spread over the
     * machine; the feedback unwrap and fit guessed in parallel and verified, else walked by one wave per channel):
     * 1 (default) = where it pays (a window class of the call with at most 64 channels and 2048 symbols or more out
     * per channel, or at most 512 channels and 24576 symbols; numAvg <= 128, samplesPerBaud 2 .. 16), 0 = never,
     * 2 = wherever the kernels exist (tests).  No effect on results.
     * The environment variable PSK_SOFT_TIME_TILED (0 / 1 / 2) sets the default of new handles. */
    PSK_SOFT_OPT_TIME_TILED = 3,
    /* The feedback unwrap and fit of a time-tiled call: 1 (default) = guessed in parallel along time and verified
     * position by position, a second round on corrected unwrap counts enqueued for a while after a call whose first
     * guess failed; 2 = the second round always enqueued; 0 = walked block by block, one wave per channel.  No effect on
     * results.  Environment: PSK_SOFT_PARALLEL_FIT. */
    PSK_SOFT_OPT_PARALLEL_FIT = 4,
    /* 1 = deferred join (default 0).  A batch that mixes window classes runs its classes on side streams of the handle.  By
     * default every call ends with the caller's stream waiting for them (results in stream order, like everything else).
     * With this option it does not: every class ends its calls on its own stream and the next call's launches of that class
     * queue behind them there, so a class with short launches runs ahead into the following calls while another is still
     * busy (configs[4] of the benchmark: 3.4 -> 2.8 ms per step).  The caller's stream -- or any stream -- sees the results of all
     * calls made so far after psk_soft_join(); psk_soft_synchronize() waits for them on the host.  Results are unchanged.
     * A call whose channels would not all stay on the stream they were on (a property or packet pattern that moves a channel
     * to another window class) joins everything first, by itself. */
    PSK_SOFT_OPT_DEFERRED_JOIN = 5,
    /* 1 = every psk_soft_process_* call ends with a reduction pass over the output rows it has just written: one
     * psk_soft_quality_t per channel of the call, read back with psk_soft_get_quality (see there).  0 (default): nothing
     * changes -- no launch, no record.  Setting the option to 1 zeroes all records.  Any other value is refused.
     * Results of the four streams are unchanged.  The pass reads the call's WHOLE rows, so they must be complete on the
     * caller's stream: with PSK_SOFT_OPT_DEFERRED_JOIN also on, the call joins its side streams before the pass, and the
     * deferred join has no effect while this option is on (the call is still cut in time and by class as before; the
     * pass comes behind the join of the last piece).  Outputs in psk_soft_host_alloc memory are read back over the link
     * by the pass: correct, and the one case where the option costs a second crossing of the soft rows. */
    PSK_SOFT_OPT_QUALITY = 6,
    /* phaseAvg 32641 .. 65535 ("far" fit windows, more than any LDS ring holds).  0 (default): a call of such a channel that
     * emits symbols runs on the reference-order kernel, one lane per channel, and the launch of the whole batch waits for it.
     * 1 = it runs on the time-tiled kernels, behind the front stage that takes samplesPerBaud and numAvg at run time, with a fit
     * stage that keeps the fit window in a scratch in device memory: 512 KiB per far channel, owned by the handle, allocated
     * when the first such call comes and kept.  Any other value is refused.  Takes effect at the next process call; results are
     * unchanged, bit for bit; psk_soft_set_force_sequential(1) still wins.  Such channels count in channels_fast and
     * channels_tiled.  The environment variable PSK_SOFT_FAR_FIT (0 / 1) sets the default of new handles. */
    PSK_SOFT_OPT_FAR_FIT = 7
};
psk_soft_status psk_soft_set_option(psk_soft_handle_t *h, int option, int value);

/* ---- which channels hold a signal (PSK_SOFT_OPT_QUALITY) ----------------------------------------------------------
 * The reference answers that question with its two debug ports: `phase` (cpp/psk_soft.cpp:482) and `sampleIndex`
 * (:466) exist so that a person can watch carrier and timing in a plot.  For thousands of channels the record below
 * stands in for the plot: sums over the soft symbols of ONE call, taken on the GPU while the rows are still in HBM,
 * and the two ends of the call's phase and sampleIndex rows.  Sums, not means, and nothing accumulates across calls:
 * a host that wants a longer average adds the sums and counts of consecutive records.
 *
 * Per soft symbol (re, im), in float32, every operation rounded once, no fused multiply-add, denormals kept:
 *   e = re*re + im*im,  q = e*e.  The symbol is FINITE when re, im and q are finite (the first symbol of a
 *   differentially decoded stream is inf / NaN -- a quotient by the zero before the stream -- and is left out).
 *   (pr, pi) = (re, im), then log2(M) times (pr, pi) <- (pr*pr - pi*pi, pr*pi + pi*pr): z^M.
 *   a = e for M = 2, q for 4, q*q for 8: |z|^M without a square root.  The symbol enters the lock sums when it is
 *   finite, pr, pi and a are finite and a >= FLT_MIN; its term is the unit phasor c = (pr / a, pi / a) (unit phasors,
 *   not amplitude-weighted ones: two or three huge quotients of a differential stream would carry a weighted sum).
 * The sums are doubles, added in a fixed order: the same call on two fresh handles gives byte-identical records. */
enum { PSK_SOFT_Q_SOFT = 1, PSK_SOFT_Q_PHASE = 2, PSK_SOFT_Q_INDEX = 4, PSK_SOFT_Q_LOCK = 8, PSK_SOFT_Q_PLANNED = 128 };

typedef struct psk_soft_quality {           /* the LAST call that covered the channel with the option on */
    uint64_t n_symbols;       /* symbols that call emitted for the channel                                   */
    uint64_t n_finite;        /* of those: soft symbols that enter sum_e / sum_e2                            */
    uint64_t n_lock;          /* of those: soft symbols that enter sum_lock_*                                */
    uint64_t index_changes;   /* i >= 1 with sampleIndex[i] != sampleIndex[i-1] (timing picks that moved)    */
    double sum_e, sum_e2;     /* sums of e_i and of q_i (above)                                              */
    double sum_lock_re, sum_lock_im;   /* sum of the unit phasors c_i (above)                                */
    float phase_first, phase_last;     /* phase[0], phase[n-1] of the call, copied                           */
    int16_t index_first, index_last;   /* sampleIndex[0], sampleIndex[n-1], copied                           */
    uint16_t constelationSize, samplesPerBaud;   /* the snapshot the call ran with                           */
    uint8_t differentialDecoding, flags;         /* PSK_SOFT_Q_*: which parts of the record are filled in    */
    uint8_t pad[6];                              /* zero; the struct is a multiple of 8 bytes                */
} psk_soft_quality_t;
/* flags of a data record: Q_SOFT when the call had a soft pointer and emitted symbols (else the four sums, n_finite and
 * n_lock are zero), Q_PHASE likewise for phase_*, Q_INDEX for index_* / index_changes (a sampleIndex pointer and
 * n_sampleIndex > 0: not at samplesPerBaud 1), Q_LOCK when Q_SOFT and constelationSize is 2, 4 or 8.  A covered channel
 * that emits nothing (no packet, real data, a window still filling) gets an all-zero record, written in stream order
 * by the pass; a channel a call does not cover keeps its record.  A control-plane-only handle fills in n_symbols, the
 * three snapshot fields and flags = PSK_SOFT_Q_PLANNED, everything else zero. */

/* lock:  |sum of the unit phasors| / n_lock -- 1 for a stream whose M-th power points one way, whatever way; of the order
 *        of n^-1/2 .. 0.1 for noise.  NaN without Q_LOCK or with n_lock 0.
 * snr_db: second- and fourth-moment estimator for a constant-modulus signal in complex Gaussian noise: m2 = sum_e / n_finite,
 *        m4 = sum_e2 / n_finite, d = 2 m2^2 - m4, s = sqrt(d), 10 log10(s / (m2 - s)); NaN when d <= 0, m2 - s <= 0, n_finite is 0
 *        or differentialDecoding (the soft symbols are quotients of two noisy samples there: heavy-tailed, the moments
 *        mean nothing; lock stays valid).  An ESTIMATE on the one sample per symbol the timing pick chose, not a
 *        calibrated measurement.
 * mean_energy: sum_e / n_finite (NaN with n_finite 0).
 * index_change_rate: index_changes / (n_symbols - 1); NaN without Q_INDEX or with fewer than two symbols. */
typedef struct psk_soft_quality_derived { double lock, snr_db, mean_energy, index_change_rate; } psk_soft_quality_derived_t;

uint64_t psk_soft_quality_bytes(void);      /* sizeof(psk_soft_quality_t), for bindings */
/* waits like psk_soft_get_channel_stats does and copies the records of [ch0, ch0+nch) out */
psk_soft_status psk_soft_get_quality(psk_soft_handle_t *h, uint32_t ch0, uint32_t nch, psk_soft_quality_t *q /* [nch] */);
psk_soft_status psk_soft_quality_derive(const psk_soft_quality_t *q, psk_soft_quality_derived_t *d);  /* host only, pure */

/* ---- carrier offset of a packet (psk_soft_acquire_device) ---------------------------------------------------------------------
 * psk_soft_process_device_tuned takes a carrier offset out; this call finds it.  The tracker of serviceFunction() sees the carrier
 * once per symbol, behind the M-th power: offsets of f and of f + 1/M cycles per SYMBOL look the same to it (and to `lock`), so no
 * search over `step` that watches `lock` can tell them apart.  The samples can: in front of the timing pick there are
 * samplesPerBaud of them per symbol, and the lag products below are unambiguous for |f| < 1/(2M) cycles per SAMPLE, which is
 * samplesPerBaud/(2M) cycles per symbol -- samplesPerBaud/2 times the tracker's range of 1/M cycles per symbol.
 *
 * The call looks at one packet per channel and leaves one record per channel.  It emits no symbols and touches no demodulator
 * state: psk_soft_peek, psk_soft_query, the state blob, warning counts, statistics, quality records and the results of every
 * later process call are what they are without it.  It ignores sriChanged and inputQueueFlushed.
 *
 * The definition.  Lags are L_j = 2^j, j = 0 .. 7 (1, 2, 4 .. 128).  M is the channel's stored constelationSize, the value the
 * next process call would snapshot.
 * Samples: the samples of the packet are converted exactly, as its format defines; if tune[i] is given and not {0, 0} they are
 *   multiplied by the NCO exactly as "tuned packets" (above) defines, bit for bit.  Call the result (re, im) of sample k.
 * Per sample, every operation float32, rounded once, no fused multiply-add, denormals kept (the terms of the lock sum of the
 *   quality record):
 *     e = re*re + im*im,  q = e*e
 *     (pr, pi) = (re, im), then log2(M) times (pr, pi) <- (pr*pr - pi*pi, pr*pi + pi*pr)
 *     a = e for M = 2, q for 4, q*q for 8
 *   Sample k is VALID when re, im, q, pr, pi and a are finite and a >= FLT_MIN.  For a valid sample u_k = (pr / a, pi / a), the
 *   division correctly rounded.  sum_e is the sum of (double)e over the valid samples, n_valid their count.
 * Per lag j, for every k >= L_j with k and k - L_j both valid (L = L_j):
 *     t_re = ur_k*ur_{k-L} + ui_k*ui_{k-L},   t_im = ui_k*ur_{k-L} - ur_k*ui_{k-L}        (float32)
 *     sum_re[j] += (double)t_re,  sum_im[j] += (double)t_im,  n_pairs[j]++
 * Order of the additions: the doubles are added in an order fixed by the code, a function of the packet's length only -- not of
 *   the batch, the grid, the stride, the format or the stream: the same samples give the same bytes whether the packet stands alone
 *   or among 4095 others.  No floating-point atomics.  (psk_soft_acquire_host adds in index order: its sums agree with the
 *   device's within n * 2^-53 * sum|t|, not bit for bit.) */
enum { PSK_SOFT_A_DATA = 1, PSK_SOFT_A_TUNED = 2, PSK_SOFT_A_PLANNED = 128 };

typedef struct psk_soft_acquire {        /* the LAST psk_soft_acquire_device call that covered the channel */
    uint64_t n_samples, n_valid;         /* complex samples of the packet; of those, valid ones            */
    uint64_t n_pairs[8];                 /* per lag: pairs that entered the sums                           */
    double sum_re[8], sum_im[8];         /* per lag: sums of t_re, t_im                                    */
    double sum_e;                        /* sum of e over the valid samples                                */
    uint16_t constelationSize; uint8_t flags; uint8_t pad[5];   /* PSK_SOFT_A_*; pad zero                  */
} psk_soft_acquire_t;                    /* 224 bytes */

/* psk_soft_acquire_derive (doubles; C atan2, hypot, rint), with c_j = |(sum_re[j], sum_im[j])| / n_pairs[j]:
 *   all three doubles NaN and lags_used 0 without PSK_SOFT_A_DATA, with n_pairs[0] == 0 or with both lag-1 sums zero.  Else
 *   f = atan2(sum_im[0], sum_re[0]) / (2 pi M), lags_used = 1; then for j = 1 .. 7, stopping at the first j with n_pairs[j] == 0
 *   or c_j < 0.5 * c_0 (a carrier that decorrelates over long lags is not trusted there; the factor is part of the definition):
 *     d = atan2(sum_im[j], sum_re[j]) - 2 pi M L_j f,  d -= 2 pi rint(d / (2 pi)),  f += d / (2 pi M L_j),  lags_used++
 *   offset_cycles_per_sample = f, coherence = c_0, mean_energy = sum_e / n_valid.
 * coherence is of the order of n^-1/2 for noise and near 1 for a clean PSK signal; where to put the threshold is the host's choice.
 * Sign: the signal's phase advances by f cycles per sample; take it out with tune.step += psk_soft_tune_step(-f).  If the look was
 * itself tuned, f is the residual under that tune.  Unambiguous for |f| < 1/(2M) cycles per sample (see the top of the section). */
typedef struct psk_soft_acquire_derived { double offset_cycles_per_sample, coherence, mean_energy; int32_t lags_used; int32_t pad; } psk_soft_acquire_derived_t;

/* Packets, strides and tunes as for psk_soft_process_device_tuned (DEVICE pointers; enqueued on `stream`, returns without
 * waiting).  Refused with PSK_SOFT_ERR_INVALID_ARG before anything is enqueued or any record changes: a bad channel range, and on
 * a present packet a stride of 0, an extent stride x bytes-per-sample x samples that does not fit 64 bits, an unknown format, or
 * `data` that is missing or not aligned to a whole sample when the packet holds samples the call would read.
 * A covered channel gets a DATA record (PSK_SOFT_A_DATA, and PSK_SOFT_A_TUNED if it was tuned) when its packet is present, has
 * sri_mode == 1 and at least one sample, and constelationSize is 2, 4 or 8; every other covered channel gets an all-zero
 * record, written in stream order; a channel the call does not cover keeps its record.
 * How: two launches on `stream`, a fold over pieces of a fixed number of samples and a join per packet.  Strided packets in a
 * run the tiled transpose takes (at least 8 adjacent columns of one matrix, as for psk_soft_process_device_strided) are first
 * gathered, by that entry's gather launches on `stream`, into rows of their own format in the handle's gather scratch, and the
 * fold reads the rows; the scratch, its events and the rule of PSK_SOFT_OPT_DEFERRED_JOIN are that entry's: a look that gathers
 * JOINS the handle's side streams into `stream` first.  Any other strided packet is read where it lies, at its stride: every
 * load a memory line of its own -- correct, and slow for long looks; keep a matrix's channels consecutive in the call.  Nothing
 * else is launched.  A control-plane-only handle checks the arguments, then fills in n_samples, constelationSize and
 * flags = PSK_SOFT_A_PLANNED for the packets that would give a data record, everything else zero. */
psk_soft_status psk_soft_acquire_device(psk_soft_handle_t *h, uint32_t ch0, uint32_t nch, const psk_soft_packet_t *pkts /* [nch] */,
                                        const uint64_t *sample_stride /* [nch], or NULL */, const psk_soft_tune_t *tune /* [nch], or NULL */,
                                        void *stream);
/* waits like psk_soft_get_quality does and copies the records of [ch0, ch0+nch) out */
psk_soft_status psk_soft_get_acquire(psk_soft_handle_t *h, uint32_t ch0, uint32_t nch, psk_soft_acquire_t *rec /* [nch] */);
psk_soft_status psk_soft_acquire_derive(const psk_soft_acquire_t *rec, psk_soft_acquire_derived_t *d);   /* host only, pure */
/* host only, pure: the definition for n_complex CF32 samples (tune NULL or {0, 0}: untuned), the sums added in index order;
 * PSK_SOFT_ERR_INVALID_ARG for a constelationSize other than 2, 4, 8 */
psk_soft_status psk_soft_acquire_host(uint16_t constelationSize, const psk_soft_tune_t *tune /* or NULL */,
                                      const float *in, uint64_t n_complex, psk_soft_acquire_t *rec);
uint64_t psk_soft_acquire_bytes(void);      /* sizeof(psk_soft_acquire_t), for bindings */
uint32_t psk_soft_acquire_piece(void);      /* samples of one piece of the device's fold (tests: the lengths at its edges) */

/* ---- symbol rate of a packet (psk_soft_symrate_device) ------------------------------------------------------------------------
 * psk_soft_process_device_resampled takes a symbol rate that does not divide the sample rate to samplesPerBaud samples a symbol;
 * this call finds the ratio.  It is the carrier look's lag ladder applied to the timing tone: the envelope of a shaped PSK signal,
 * and the transition energy of a rectangular one, carry a line at the symbol rate; folded over blocks of S = samplesPerBaud
 * samples that line turns by f = S/sps - 1 cycles from one block to the next, and the lag products of the block sums measure f.
 *
 * The call looks at one packet per channel and leaves one record per channel.  It emits no symbols, keeps no history and touches
 * no demodulator state, resampler history or filter history: psk_soft_peek, psk_soft_query, the state blob, warning counts,
 * statistics, quality records, carrier-look records and the results of every later process call are what they are without it.
 * It ignores sriChanged and inputQueueFlushed.
 *
 * The definition.  S is the channel's stored samplesPerBaud, the value the next process call would snapshot.  Lags are L_j = 2^j
 * blocks, j = 0 .. 7.
 * Samples: converted, and tuned if tune[i] is given and not {0, 0}, exactly as for psk_soft_acquire_device.  Call the result
 *   (re, im) of sample k.  The look uses the first n_used = min(n, 4096 S) samples rounded down to whole blocks of S samples:
 *   n_blocks = min(n, 4096 S) / S, n_used = n_blocks S.  Block m holds the samples k = m S + p, p = 0 .. S - 1.
 * Per sample, every operation float32, rounded once, no fused multiply-add, denormals kept -- two detectors of the line:
 *     e_k = re*re + im*im                                                   (the envelope: shaped pulses)
 *     g_k = dr*dr + di*di,  dr = re_k - re_{k-1},  di = im_k - im_{k-1};  g_0 = 0  (the transition energy: rectangular pulses)
 * Per position p: (c_p, s_p) is the phasor W that "tuned packets" (above) defines for the phase word
 *   (0 - p * floor(2^64 / S)) mod 2^64 -- the two table entries multiplied as there.  It restarts in every block and does not drift.
 * Per block m and detector z in {e, g} (index 0, 1):
 *     B_z[m] = (sum_p (double)(z_k * c_p), sum_p (double)(z_k * s_p))      the products float32, the sums double
 *   A block is VALID when all its samples are finite, the sample in front of its first one is finite if there is one, and all
 *   its e and g are finite.  An invalid block enters nothing.  Over the valid blocks: sum_pow[z] = sum of
 *   Br*Br + Bi*Bi (doubles, no fused multiply-add), sum_lvl[z] = sum of (double)z_k over their samples, n_valid their count.
 * Per lag j, for every m >= L_j with blocks m and m - L_j both valid (a = B_z[m], b = B_z[m - L_j]; doubles, no fused multiply-add):
 *     sum_re[z][j] += ar*br + ai*bi,  sum_im[z][j] += ai*br - ar*bi;  n_pairs[j]++ (the same for both detectors)
 * Order of the additions: fixed by the code, a function of (n_used, S) only -- not of the batch, the grid, the stride, the format
 *   or the stream: the same samples give the same bytes whether the packet stands alone or among 4095 others.  No floating-point
 *   atomics.  (psk_soft_symrate_host adds in index order: its sums agree with the device's within n * 2^-53 * sum|t| -- for the
 *   lag sums with the block sums' own error of S * 2^-53 * sum|term| carried through the product --, not bit for bit.) */
enum { PSK_SOFT_SR_DATA = 1, PSK_SOFT_SR_TUNED = 2, PSK_SOFT_SR_PLANNED = 128 };

typedef struct psk_soft_symrate {        /* the LAST psk_soft_symrate_device call that covered the channel */
    uint64_t n_samples, n_used;          /* complex samples of the packet; of those, the ones the look used */
    uint64_t n_blocks, n_valid;          /* n_used / samplesPerBaud; of those, valid ones                   */
    uint64_t n_pairs[8];                 /* per lag: pairs of blocks that entered the sums                  */
    double sum_re[2][8], sum_im[2][8];   /* per detector (0: e, 1: g) and lag: sums of the lag products     */
    double sum_pow[2], sum_lvl[2];       /* per detector: sum of |B|^2, sum of z, over the valid blocks     */
    uint16_t samplesPerBaud; uint8_t flags; uint8_t pad[5];     /* PSK_SOFT_SR_*; pad zero                 */
} psk_soft_symrate_t;                    /* 392 bytes */

/* psk_soft_symrate_derive (doubles; C atan2, hypot, rint).  Per detector z, with p_z = sum_pow[z] / n_valid the mean power of a
 * block sum:  c_j[z] = |(sum_re[z][j], sum_im[z][j])| / (n_pairs[j] * p_z); c_0[z] = 0 for a detector whose lag-1 sums are both
 * zero.  The detector with the larger c_0 answers, a tie goes to e (detector = 0).
 *   All doubles NaN, detector -1 and lags_used 0 without PSK_SOFT_SR_DATA, with n_pairs[0] == 0 or with the lag-1 sums of both
 *   detectors zero.  Else, on the chosen detector,
 *   f = atan2(sum_im[0], sum_re[0]) / (2 pi), lags_used = 1; then for j = 1 .. 7, stopping at the first j with n_pairs[j] < 8 or
 *   c_j < 0.5 * c_0 (the factor is part of the definition):
 *     d = atan2(sum_im[j], sum_re[j]) - 2 pi L_j f,  d -= 2 pi rint(d / (2 pi)),  f += d / (2 pi L_j),  lags_used++
 *   samples_per_symbol = S / (1 + f), step_ratio = 1 / (1 + f) -- what psk_soft_resample_step takes to bring the signal to S samples
 *   a symbol --, coherence = c_0, mean_level = sum_lvl / (n_valid * S) of the chosen detector.
 * Range: f is unambiguous for |f| < 1/2, but the USEFUL range is a symbol rate within about +-20 % of S samples a symbol: the
 * line's image at -1/sps leaks through the block sum beyond that and pulls the estimate (11.0 at S = 8 and 5.2 at S = 4 fail).
 * coherence is of the order of n_blocks^-1/2 for noise and near 1 for a clean signal; the threshold is the host's choice.
 * Which detector answers: e for band-limited (shaped) pulses, whose envelope dips between symbols; g for rectangular pulses,
 * whose envelope is flat (c_0[e] ~ noise) and whose only trace of the symbol clock is the jump at a transition. */
typedef struct psk_soft_symrate_derived { double samples_per_symbol, step_ratio, coherence, mean_level; int32_t detector, lags_used; } psk_soft_symrate_derived_t;

/* Packets, strides and tunes as for psk_soft_acquire_device, and its refusals (PSK_SOFT_ERR_INVALID_ARG before anything is enqueued
 * or any record changes): a bad channel range, and on a present packet a stride of 0, an extent that does not fit 64 bits, an
 * unknown format, or `data` that is missing or not aligned to a whole sample when the packet holds samples the call would read.
 * A covered channel gets a DATA record (PSK_SOFT_SR_DATA, and PSK_SOFT_SR_TUNED if it was tuned) when its packet is present, has
 * sri_mode == 1, 4 <= samplesPerBaud <= 1024 and at least 2 samplesPerBaud samples; every other covered channel gets an all-zero
 * record, written in stream order; a channel the call does not cover keeps its record.
 * How: two launches on `stream`, a fold over pieces of a fixed number of blocks (the 128 blocks in front of a piece are computed
 * again; the block sums stay in LDS) and a join per packet.  Strided packets go through the gather exactly as the carrier look's
 * do -- the first n_used samples of a column of a run of at least 8, any other strided packet read where it lies --, with that
 * entry's scratch, events and rule of PSK_SOFT_OPT_DEFERRED_JOIN.  Nothing else is launched.  A control-plane-only handle checks
 * the arguments, then fills in n_samples, n_used, n_blocks, samplesPerBaud and flags = PSK_SOFT_SR_PLANNED for the packets that
 * would give a data record, everything else zero. */
psk_soft_status psk_soft_symrate_device(psk_soft_handle_t *h, uint32_t ch0, uint32_t nch, const psk_soft_packet_t *pkts /* [nch] */,
                                        const uint64_t *sample_stride /* [nch], or NULL */, const psk_soft_tune_t *tune /* [nch], or NULL */,
                                        void *stream);
/* waits like psk_soft_get_acquire does and copies the records of [ch0, ch0+nch) out */
psk_soft_status psk_soft_get_symrate(psk_soft_handle_t *h, uint32_t ch0, uint32_t nch, psk_soft_symrate_t *rec /* [nch] */);
psk_soft_status psk_soft_symrate_derive(const psk_soft_symrate_t *rec, psk_soft_symrate_derived_t *d);   /* host only, pure */
/* host only, pure: the definition for n_complex CF32 samples (tune NULL or {0, 0}: untuned), the sums added in index order; the
 * zero record for n_complex < 2 samplesPerBaud; PSK_SOFT_ERR_INVALID_ARG for a samplesPerBaud outside 4 .. 1024 */
psk_soft_status psk_soft_symrate_host(uint16_t samplesPerBaud, const psk_soft_tune_t *tune /* or NULL */,
                                      const float *in, uint64_t n_complex, psk_soft_symrate_t *rec);
uint64_t psk_soft_symrate_bytes(void);      /* sizeof(psk_soft_symrate_t), for bindings */
uint32_t psk_soft_symrate_piece(void);      /* blocks of one piece of the device's fold (tests: the lengths at its edges) */

/* ---- where frames start: a known word in the soft symbols (psk_soft_sync_device) ----------------------------------------------
 * The M-th-power tracker leaves the constellation turned by an unknown multiple of 2 pi / M and nothing in the four streams says
 * where a frame starts.  A receiver slides a word it knows (unique word, preamble, sync marker) along the soft symbols: the
 * correlation peak gives the frame start, the peak's angle the rotation.  This call does that on the GPU over rows that are
 * already in device memory -- typically the `soft` rows of the process call enqueued on the same stream just before -- and leaves
 * one small record per channel.
 *
 * The call touches no demodulator state, statistics, quality or look records and no filter or resampler history: psk_soft_peek,
 * psk_soft_query, the state blob, warning counts, statistics and the results of every later process call are what they are
 * without it.  The rows are read, never written.
 *
 * Words.  The handle keeps PSK_SOFT_SYNC_SLOTS numbered words (psk_soft_sync_define): L = 1 .. PSK_SOFT_SYNC_MAX_WORD complex
 *   float32 points w[0] .. w[L-1], interleaved (re, im), as the caller expects them in `soft`.
 *   Ew = the float32 sum, in index order, of w.re*w.re + w.im*w.im (each term rounded, then added; the sum starts from term 0).
 * Input.  One psk_soft_sync_in_t per covered channel: n = n_symbols (re, im) pairs at `soft`, x[0] .. x[n-1].
 * History.  x[-127] .. x[-1] are the channel's HISTORY: the last PSK_SOFT_SYNC_MAX_WORD - 1 soft symbols of its stream in front
 *   of this row, oldest first; zeros with PSK_SOFT_SYNC_RESTART.  It always holds 127 symbols, whatever L.
 * Windows.  Window p covers x[p] .. x[p + L - 1].  p runs from p0 to n - L, p0 = 0 with PSK_SOFT_SYNC_RESTART (no window starts in
 *   front of the row) and -(L - 1) otherwise; n_windows = n - L - p0 + 1, or 0 if n - L < p0.  Every symbol position of a
 *   continuous stream so starts exactly one window across its calls.
 * Per window -- every operation float32, rounded once, no fused multiply-add, denormals kept; j = 0 .. L-1 in that order, the
 *   accumulators starting from the j = 0 term:
 *     tr = x[p+j].re*w[j].re + x[p+j].im*w[j].im     ti = x[p+j].im*w[j].re - x[p+j].re*w[j].im     te = x.re*x.re + x.im*x.im
 *     cr += tr;  ci += ti;  e += te
 *   then  q = cr*cr + ci*ci,  d = e*Ew,  m = q / d  (the division correctly rounded): the squared correlation over the product of
 *   the energies, 1 for a window that is the word times any complex factor, by Cauchy-Schwarz never above 1 but for rounding.
 *   The window is VALID when cr, ci, e, q and d are finite and d >= FLT_MIN; a HIT when it is valid and m >= threshold; the BEST
 *   window is the valid one with the greatest m, the first such on a tie.
 * Every term is float32 in a fixed order per window, so no reduction order enters any stored value: psk_soft_sync_host and the
 *   device agree byte for byte, and the same symbols give the same bytes whatever the batch, the grid or the stream.
 * After the call the history is the last 127 of (old history || row), zeros for the old history with PSK_SOFT_SYNC_RESTART.  A
 *   short first row after a restart therefore leaves zeros in the history, and the windows of the NEXT call that reach into them
 *   correlate against those zeros: they are the host's to drop -- it knows its stream offset (positions below -(symbols since
 *   the restart)).  The history is not part of the state blob; psk_soft_sync_get_history / _set_history carry it. */
#define PSK_SOFT_SYNC_MAX_WORD 128
#define PSK_SOFT_SYNC_SLOTS    16
#define PSK_SOFT_SYNC_HITS     16
enum { PSK_SOFT_SYNC_RESTART = 1 };                          /* psk_soft_sync_in_t.flags */
enum { PSK_SOFT_SYNC_DATA = 1, PSK_SOFT_SYNC_PLANNED = 128 }; /* psk_soft_sync_t.flags    */

typedef struct psk_soft_sync_in {
    const float *soft;    /* DEVICE pointer: n_symbols (re, im) pairs, 8-byte aligned; NULL: not searched                  */
    uint64_t n_symbols;   /* below 2^30; 0: not searched                                                                   */
    uint32_t word;        /* 1 + the slot of the word; 0: not searched                                                     */
    uint32_t flags;       /* PSK_SOFT_SYNC_RESTART: the history in front of the row is zeros, no window starts in front    */
    float threshold;      /* a hit is a valid window with m >= threshold; in (0, 1]                                        */
    uint32_t pad;         /* zero                                                                                          */
} psk_soft_sync_in_t;     /* 32 bytes */

typedef struct psk_soft_sync_hit {
    int64_t pos;          /* p, relative to the row's symbol 0: negative for a window that starts in the history           */
    float cr, ci, e, m;   /* the window's sums and its metric                                                              */
} psk_soft_sync_hit_t;    /* 24 bytes */

typedef struct psk_soft_sync {           /* the LAST psk_soft_sync_device call that covered the channel */
    uint64_t n_symbols, n_windows;       /* symbols of the row; windows searched                                           */
    uint64_t n_valid, n_hits;            /* of those, valid ones; of those, hits (all of them, not only the stored ones)   */
    psk_soft_sync_hit_t best;            /* the best window; all-zero bytes without a valid window                         */
    psk_soft_sync_hit_t hits[PSK_SOFT_SYNC_HITS];   /* the first 16 hits in position order; unused ones all-zero bytes    */
    uint32_t word_len, flags;            /* L; PSK_SOFT_SYNC_DATA or PSK_SOFT_SYNC_PLANNED                                 */
    uint32_t pad[2];                     /* zero                                                                           */
} psk_soft_sync_t;                       /* 456 bytes */

/* The word of slot `slot` (0 .. PSK_SOFT_SYNC_SLOTS - 1): n = 1 .. PSK_SOFT_SYNC_MAX_WORD points (2 n floats), copied into device
 * memory the handle owns; a searched channel names it as word = slot + 1.  Redefining a slot waits for the handle's last sync
 * launch first.  A control-plane-only handle records the length only.  PSK_SOFT_ERR_INVALID_ARG: null pointer, slot or n out of
 * range. */
psk_soft_status psk_soft_sync_define(psk_soft_handle_t *h, uint32_t slot, const float *word, uint32_t n);

/* The search of in[i] for channel ch0 + i.  The rows must be complete on `stream` (a process call enqueued there just before
 * is: no synchronize lies between the two); with PSK_SOFT_OPT_DEFERRED_JOIN pending the call joins the side streams into `stream`
 * first, exactly as the quality pass does.  The call returns without waiting.
 * A covered channel with word == 0, soft == NULL or n_symbols == 0 is not searched: it gets an all-zero record, written in stream
 * order, and its history does not move.  A channel the call does not cover keeps record and history.
 * Refusals (PSK_SOFT_ERR_INVALID_ARG before anything is enqueued, any record changes or any history flips): a bad channel range,
 * a null pointer; on a searched channel a slot >= 16 or never defined, a threshold that is NaN, <= 0 or > 1, unknown flag bits,
 * a non-zero pad, a `soft` that is not 8-byte aligned, n_symbols >= 2^30.
 * How: two launches on `stream`.  The fold's grid is pieces x channels; a piece is a fixed number of windows
 * (psk_soft_sync_piece), staged with the L - 1 symbols behind them and the word in LDS, consecutive lanes taking consecutive
 * windows; each piece leaves its counts, its best and its first 16 hits (compacted in position order by ballot and prefix
 * count: no atomics decide an order), and piece 0 writes the channel's new history into its other slot.  The join, one wave per
 * channel, walks the pieces in order and writes the record.  The histories flip when the whole call returned PSK_SOFT_OK.
 * A control-plane-only handle checks the arguments, then fills in n_symbols, n_windows, word_len and flags =
 * PSK_SOFT_SYNC_PLANNED for the searched channels, everything else zero. */
psk_soft_status psk_soft_sync_device(psk_soft_handle_t *h, uint32_t ch0, uint32_t nch, const psk_soft_sync_in_t *in /* [nch] */,
                                     void *stream);
/* waits like psk_soft_get_quality does and copies the records of [ch0, ch0+nch) out */
psk_soft_status psk_soft_get_sync(psk_soft_handle_t *h, uint32_t ch0, uint32_t nch, psk_soft_sync_t *rec /* [nch] */);
/* the history of a channel -- 127 (re, im) pairs, oldest first -- read or replaced behind the last sync launch (zeros before the
 * first; a control-plane-only handle keeps zeros) */
psk_soft_status psk_soft_sync_get_history(psk_soft_handle_t *h, uint32_t ch, float *out /* [254] */);
psk_soft_status psk_soft_sync_set_history(psk_soft_handle_t *h, uint32_t ch, const float *in /* [254] */);

/* psk_soft_sync_derive (host only, pure, doubles; C atan2, rint, sqrt) of one hit, for constelationSize M, word length L and the
 * word's Ew:  angle = atan2(ci, cr);  rotation = rint(angle M / (2 pi)) mod M, in 0 .. M-1: the multiple of 2 pi / M by which the
 * symbols are turned against the word;  residual = angle - rint(angle M / (2 pi)) 2 pi / M, within +-pi / M;  amplitude =
 * sqrt(e / L), the rms symbol amplitude of the window;  metric = (cr*cr + ci*ci) / (e * Ew), the hit's m formed again in doubles.  An all-zero hit gives NaN everywhere and rotation -1.  A
 * different rotation at two frames of one stream is a cycle slip of the tracker between them.  The positions are relative to each
 * call's row: the host keeps the absolute symbol count (add n_symbols of every call).
 * PSK_SOFT_ERR_INVALID_ARG: null pointer, M other than 2, 4, 8, L outside 1 .. 128. */
typedef struct psk_soft_sync_derived { double angle, residual, amplitude, metric; int32_t rotation, pad; } psk_soft_sync_derived_t;
psk_soft_status psk_soft_sync_derive(const psk_soft_sync_hit_t *hit, uint16_t constelationSize, uint32_t word_len, float Ew,
                                     psk_soft_sync_derived_t *out);
/* host only, pure: the definition for one row on the host.  hist_in NULL or PSK_SOFT_SYNC_RESTART: a history of zeros; hist_out
 * (may be NULL) receives the history behind the row; *rec and hist_out are byte for byte what the device writes (flags =
 * PSK_SOFT_SYNC_DATA).  n == 0 gives the zero record and hist_out = the history in front.  Refuses what the entry refuses of
 * L, threshold, flags and n. */
psk_soft_status psk_soft_sync_host(const float *word, uint32_t L, float threshold, uint32_t flags, const float *hist_in /* [254] or NULL */,
                                   const float *soft, uint64_t n, psk_soft_sync_t *rec, float *hist_out /* [254] or NULL */);
uint64_t psk_soft_sync_bytes(void);         /* sizeof(psk_soft_sync_t), for bindings */
uint64_t psk_soft_sync_in_bytes(void);      /* sizeof(psk_soft_sync_in_t), for bindings */
uint32_t psk_soft_sync_piece(void);         /* windows of one piece of the device's fold (tests: the counts at its edges) */

/* ---- frames as soft bits: segments of the soft rows as per-bit LLRs (psk_soft_demap_device) -------------------------------------
 * psk_soft_sync_derive says at which symbol a frame starts and by which multiple of 2 pi / M the constellation is turned.  A
 * decoder behind the demodulator eats per-bit soft decisions, not complex points.  This call cuts segments out of rows that are
 * already in device memory, turns each by a complex gain, forms max-log LLRs against a constellation the caller defines and writes
 * them where the caller wants them, as float32 or as saturated int8; it leaves one small record per segment, from which the
 * host gets the noise level that scales the next frame's LLRs.  A frame is one segment, or one segment per row it lies across.
 *
 * The call touches no demodulator state, statistics, quality, look or sync records and no history: psk_soft_peek, psk_soft_query,
 * the state blob, the statistics and the results of every later call are what they are without it.  The rows, the sync history and
 * the maps are read, never written.
 *
 * All arithmetic is float32, every operation rounded once, no fused multiply-add, denormals kept, unless doubles are named.
 * Maps.  The handle keeps PSK_SOFT_DEMAP_SLOTS numbered maps (psk_soft_demap_define): M = 2, 4 or 8 finite complex float32 points
 *   p[0] .. p[M-1], interleaved (re, im), as the caller expects them in `soft` at rotation 0, and labels[k], the B-bit label of
 *   point k, B = log2 M; the labels are a permutation of 0 .. M-1, so every bit has points on both sides.  Bit j (j = 0 .. B-1)
 *   of a symbol is (label >> (B-1-j)) & 1: MSB first.
 * Segments.  One psk_soft_demap_in_t per segment: symbol i of the segment is symbol pos + i of the row of n_symbols (re, im) pairs
 *   at `soft`; pos + count <= n_symbols.  Without PSK_SOFT_DEMAP_FRONT pos >= 0.  With it pos >= -127, and the positions -127 .. -1
 *   are the sync history in front of the row that the LAST psk_soft_sync_device call over `channel` searched -- the history that
 *   call read (zeros if it had PSK_SOFT_SYNC_RESTART) --, which is what lets a frame be cut whose word that call found at a negative
 *   position.  The handle remembers per channel whether the last sync call that covered it searched it, and with which flags;
 *   FRONT on any other channel is refused (a sync call that fails after its launches began leaves its channels not searched).
 *   The caller enqueues the demap on the stream of that sync call and ahead of the next sync call over the channel: that ordering
 *   is the caller's and is not checked.
 * Per symbol x, with g = (gain_re, gain_im):
 *     y.re = x.re*g.re - x.im*g.im     y.im = x.re*g.im + x.im*g.re     (the two products rounded, then the sum or difference)
 *     e = y.re*y.re + y.im*y.im
 *     for k = 0 .. M-1:  dr = y.re - p[k].re,  di = y.im - p[k].im,  d[k] = dr*dr + di*di
 *   A minimum over a set of k is the FIRST minimum, k ascending from the set's first member: a later one must compare less, so a
 *   NaN in the first member stays.  dmin is that minimum over all k; for each bit j
 *     l = min{d[k] : bit j of label k is 1} - min{d[k] : bit j is 0},    v = l * scale
 *   so a positive v means bit 0 is the nearer.
 * Output.  Value i*B + j of the segment is v of bit j of symbol i.  float32: ((float *)out)[i*B + j] = v as it is, but a NaN as
 *   the quiet NaN 0x7fc00000 (sign and payload of a NaN differ between machines; the bytes must not); `out` 4-byte aligned.
 *   With PSK_SOFT_DEMAP_I8: ((int8_t *)out)[i*B + j] = rintf(v) (ties to even), clamped to -127 .. 127, a NaN written as 0; `out`
 *   may have any byte alignment, so the segments of one frame abut in the frame's buffer.  Exactly count*B values are written and
 *   no byte outside them.  The outputs of a call's segments must not overlap: that is the caller's duty and is not checked.
 * Record.  One psk_soft_demap_t per segment of the LAST call, in the order of `in`.  A symbol is FINITE when y.re, y.im, e and dmin
 *   are all finite.  sum_e and sum_err add e and dmin of the finite symbols, each term widened exactly to double, in a fixed order
 *   that depends on the symbol's index in the segment only: pieces of psk_soft_demap_piece() = 1024 symbols; lane t of 256 adds
 *   its symbols t, t + 256, t + 512, t + 768 of the piece in that order, from 0.0; a xor tree across each wave of 64 lanes, offsets
 *   32 .. 1 (every lane: s += the s of lane ^ offset); the four waves in order, from wave 0's value; the pieces in ascending
 *   order, from piece 0's.  No floating-point atomics.  Because the order depends on the segment only, a frame cut into two
 *   segments gives two records whose counts add, but whose sums need not equal -- to the last bits -- the sums of the frame
 *   demapped as one segment.  sigma^2 = sum_err / (2 n_finite) is the decision-directed noise power per component. */
#define PSK_SOFT_DEMAP_SLOTS        16
#define PSK_SOFT_DEMAP_MAX_SEGMENTS (1u << 20)
enum { PSK_SOFT_DEMAP_I8 = 1, PSK_SOFT_DEMAP_FRONT = 2 };                           /* psk_soft_demap_in_t.flags */
/* psk_soft_demap_t.flags: DATA or PLANNED, ORed with REC_I8 -- the segment's PSK_SOFT_DEMAP_I8 bit shifted left by one */
enum { PSK_SOFT_DEMAP_DATA = 1, PSK_SOFT_DEMAP_REC_I8 = 2, PSK_SOFT_DEMAP_PLANNED = 128 };
enum { PSK_SOFT_DEMAP_GAIN_RESIDUAL = 1, PSK_SOFT_DEMAP_GAIN_UNIT = 2 };            /* psk_soft_demap_gain flags */

typedef struct psk_soft_demap_in {
    const float *soft;    /* DEVICE pointer to the row's symbol 0, 8-byte aligned; NULL: the segment is skipped             */
    uint64_t n_symbols;   /* length of that row; below 2^30                                                                */
    int64_t pos;          /* first symbol of the segment, relative to the row                                              */
    void *out;            /* DEVICE pointer to the output: count*B float32 (4-byte aligned) or int8 (any alignment)        */
    uint32_t count;       /* symbols in the segment; 0: the segment is skipped                                             */
    uint32_t channel;     /* used only with PSK_SOFT_DEMAP_FRONT: the channel whose sync history lies in front of the row   */
    uint32_t map;         /* 1 + the slot of the map; 0: the segment is skipped                                            */
    uint32_t flags;       /* PSK_SOFT_DEMAP_I8, PSK_SOFT_DEMAP_FRONT                                                       */
    float gain_re, gain_im;   /* the complex gain; finite                                                                  */
    float scale;          /* the LLR scale; finite                                                                         */
    uint32_t pad;         /* zero                                                                                          */
} psk_soft_demap_in_t;    /* 64 bytes */

typedef struct psk_soft_demap {          /* one per segment of the LAST psk_soft_demap_device call */
    uint64_t n_symbols;                  /* the segment's count                                                            */
    uint64_t n_finite;                   /* symbols whose y.re, y.im, e and dmin are all finite                            */
    uint64_t n_clip;                     /* int8 values the clamp changed (+-inf counts); 0 for float32                    */
    uint64_t n_nan;                      /* output values that were NaN                                                    */
    double sum_e, sum_err;               /* sums of e and of dmin over the finite symbols, in the order above              */
    uint32_t bits, flags;                /* B; PSK_SOFT_DEMAP_DATA or _PLANNED, | PSK_SOFT_DEMAP_REC_I8 for an int8 segment */
    uint32_t pad[2];                     /* zero                                                                           */
} psk_soft_demap_t;                      /* 64 bytes */

/* The map of slot `slot` (0 .. PSK_SOFT_DEMAP_SLOTS - 1), copied into memory the handle owns; a segment names it as map = slot + 1.
 * Redefining a slot waits for the handle's last demap launch first.  A control-plane-only handle records M only.
 * PSK_SOFT_ERR_INVALID_ARG: null pointer, slot out of range, M other than 2, 4, 8, a non-finite point, labels that are not a
 * permutation of 0 .. M-1. */
psk_soft_status psk_soft_demap_define(psk_soft_handle_t *h, uint32_t slot, uint32_t M, const float *points /* [2 M] */,
                                      const uint8_t *labels /* [M] */);

/* The segments in[0 .. nseg-1], nseg = 1 .. PSK_SOFT_DEMAP_MAX_SEGMENTS: the call covers segments, not channels.  The rows must be
 * complete on `stream` (a process call and a sync call enqueued there just before are); with PSK_SOFT_OPT_DEFERRED_JOIN pending
 * the call joins the side streams into `stream` first, as the sync entry does.  The call returns without waiting.  The records live
 * in memory the handle owns, grown on demand; every call replaces them.
 * A segment with count == 0, map == 0 or soft == NULL is skipped: it gets the all-zero record, nothing is written to its `out`
 * and nothing else of it is looked at.
 * Refusals (PSK_SOFT_ERR_INVALID_ARG before anything is enqueued or any record changes): a null pointer, nseg out of range; on a
 * segment that is not skipped a slot out of range or never defined, unknown flag bits, a non-zero pad, a `soft` that is not
 * 8-byte aligned, a null `out` or one that is not 4-byte aligned for float32, n_symbols >= 2^30, pos + count > n_symbols,
 * pos < 0 without PSK_SOFT_DEMAP_FRONT or pos < -127 with it, FRONT on a channel out of range or on one whose last covering sync
 * call did not search it, a gain or scale that is not finite.
 * How: two launches on `stream`.  The fold's grid is pieces x segments (more than 65535 segments take further trips of the segment
 * loop); consecutive lanes take consecutive symbols with one 8-byte load each, the map is wave-uniform, the values are staged in
 * LDS and stored as full dwords, with byte stores only at the unaligned head and tail of an int8 piece.  The join, one wave per
 * segment, adds the pieces' partials in order and writes the record.
 * A control-plane-only handle checks the arguments, then leaves records with n_symbols, bits and flags = PSK_SOFT_DEMAP_PLANNED
 * (| PSK_SOFT_DEMAP_REC_I8), everything else zero. */
psk_soft_status psk_soft_demap_device(psk_soft_handle_t *h, uint32_t nseg, const psk_soft_demap_in_t *in /* [nseg] */, void *stream);
/* waits like psk_soft_get_sync does and copies the records of the segments [first, first + n) of the last call out.
 * PSK_SOFT_ERR_INVALID_ARG: a null pointer, n == 0, a range beyond the last call's nseg, no call yet. */
psk_soft_status psk_soft_get_demap(psk_soft_handle_t *h, uint32_t first, uint32_t n, psk_soft_demap_t *rec /* [n] */);

/* host only, pure: the definition for one segment on the host.  `in` is read as the entry reads it, with HOST pointers in soft and
 * out; map and channel are not looked at (the map is points / labels / M); with PSK_SOFT_DEMAP_FRONT the positions in front of the
 * row come from front[254] (127 (re, im) pairs, oldest first), zeros if it is NULL.  The bytes at out and *rec are byte for byte
 * what the device writes (flags = PSK_SOFT_DEMAP_DATA | REC_I8).  A skipped segment gives the zero record.  Refuses what the
 * entry and psk_soft_demap_define refuse of their arguments. */
psk_soft_status psk_soft_demap_host(const float *points, const uint8_t *labels, uint32_t M, const psk_soft_demap_in_t *in,
                                    const float *front /* [254] or NULL */, psk_soft_demap_t *rec);
/* host only, pure, doubles rounded once at the end: the gain that undoes a derived hit, gain = exp(-i theta) / amplitude.
 * theta = d->rotation * 2 pi / M, its cosine and sine from an exact table (0, +-1, +-(double)M_SQRT1_2), so quadrant turns are exact;
 * with PSK_SOFT_DEMAP_GAIN_RESIDUAL theta is turned further by d->residual (C cos and sin); PSK_SOFT_DEMAP_GAIN_UNIT leaves the
 * division by d->amplitude out.  PSK_SOFT_ERR_INVALID_ARG: null pointer, M other than 2, 4, 8, unknown flags, a rotation outside
 * 0 .. M-1 (the -1 of an all-zero hit), an amplitude that is not finite and positive, with GAIN_RESIDUAL a residual that is
 * not finite. */
psk_soft_status psk_soft_demap_gain(const psk_soft_sync_derived_t *d, uint32_t M, uint32_t flags, float gain[2]);
uint64_t psk_soft_demap_bytes(void);        /* sizeof(psk_soft_demap_t), for bindings */
uint64_t psk_soft_demap_in_bytes(void);     /* sizeof(psk_soft_demap_in_t), for bindings */
uint32_t psk_soft_demap_piece(void);        /* symbols of one piece of the device's fold: the summation order's unit */

/* ---- frames as payload bits: Viterbi decoding of int8 LLR frames (psk_soft_viterbi_device) ---------------------------------------
 * What stands behind the demapper is an FEC decoder.  This call decodes frames of int8 LLRs that are already in device memory --
 * as psk_soft_demap_device writes them with PSK_SOFT_DEMAP_I8 -- with a binary convolutional code the caller defines, and writes
 * the payload bits where the caller wants them; it leaves one small record per frame.  Everything is integer arithmetic, so the
 * host definition (psk_soft_viterbi_host) and the device agree to the byte without any care about rounding.
 *
 * The call touches no demodulator state, statistics or history, and no quality, look, sync or demap record.  The LLRs and the
 * codes are read, never written.
 *
 * Code.  Constraint length K = 3 .. 7; n = 2 .. 4 generator polynomials g[j], each a K-bit integer whose bit K-1 taps the current
 *   input bit (the usual octal notation: 0171, 0133 for K = 7).  A state is K-1 bits, s = (u_t, u_{t-1}, ...) with the newest
 *   input at bit K-2.  At step t from state s_{t-1} with input u the register is r = (u << (K-1)) | s_{t-1}; code bit j is
 *   c_j = parity(r & g[j]); the new state is s_t = r >> 1.  Refused: a polynomial that is 0 or has bits at or above K, and a set
 *   of polynomials that, taken over all j, taps neither bit K-1 nor bit 0.
 * Puncturing.  A period P (1 .. 16 steps, n*P <= 32) and a `keep` mask of n*P bits: bit p*n + j set means code bit j of a step
 *   with t mod P == p was transmitted.  The frame's LLRs are the kept code bits in order of (t, j); a bit that was not kept
 *   contributes 0 and is not read.  `keep` has at least one bit set and none at or above n*P.  P = 1, keep = 2^n - 1 is the
 *   unpunctured code.  psk_soft_viterbi_count gives the number of LLRs a frame of n_steps steps holds.
 * Input.  int8 LLRs; a positive value means bit 0 is the nearer.  The pointer may have any byte alignment (the segments of a
 *   frame abut).  The value -128 is taken as it is.  float32 LLRs are not accepted by this entry.
 * Path metrics are int32 and are MAXIMISED.  The branch metric of a branch with code bits c is bm = sum_j (c_j ? -l_j : +l_j)
 *   over the kept bits.  At the start pm[0] = 0 and pm[s] = -2^30 for every other s; with PSK_SOFT_VITERBI_ANY_START every
 *   pm[s] = 0 (a frame cut out of a running stream).  n_steps <= PSK_SOFT_VITERBI_MAX_STEPS = 65536, so |pm| <= 4*128*65536 = 2^25
 *   < 2^26 on reachable states; an unreachable state stays below -2^30 + 2^26 and above -2^31.  No normalisation exists and none
 *   is needed.
 * Add-compare-select.  State s has the two predecessors p_b = ((s << 1) & (2^(K-1) - 1)) | b, b = 0, 1; its input bit is
 *   u = s >> (K-2).  pm'[s] = max_b (pm[p_b] + bm_b); b = 1 wins only if strictly greater.  The decision d_t[s] is the winning b.
 * End and traceback.  With PSK_SOFT_VITERBI_TERMINATED the end state is 0 and the last K-1 steps are the tail: n_bits =
 *   n_steps - (K-1); n_steps < K-1 is refused.  Without it the end state is the FIRST maximum of the final metrics, s ascending,
 *   and n_bits = n_steps.  Going back from t = n_steps - 1: u_t = s_t >> (K-2), s_{t-1} = ((s_t << 1) & mask) | d_t[s_t].  The
 *   state reached in front of step 0 is the record's start_state; it is 0 unless ANY_START.
 * Output.  The bits u_0 .. u_{n_bits-1}, one a byte (uint8 0 / 1).  With PSK_SOFT_VITERBI_PACKED eight a byte: bit i goes to byte
 *   i >> 3 at bit 7 - (i & 7); the unused low bits of the last byte are zero.  `out` may have any byte alignment.  Exactly n_bits,
 *   or ceil(n_bits / 8), bytes are written and no byte outside them.  The outputs of a call's frames must not overlap: that is
 *   the caller's duty and is not checked.
 * Record.  One psk_soft_viterbi_t per frame of the LAST call, in the order of `in`.  Everything in it is an integer and therefore
 *   independent of any summation order.  With start state 0 (no ANY_START) metric <= sum_abs, with equality exactly when
 *   n_flip == 0.
 * Cost.  One frame never uses more than one wave of 64 lanes, a state a lane: a call with few frames is slow, and only a call
 *   of thousands of frames fills the machine.  The decisions of a frame in flight live in scratch the handle owns, 8 bytes a
 *   step, grown on demand; a call keeps at most PSK_SOFT_VITERBI_SCRATCH_BYTES of them in flight (the allocation itself has a
 *   quarter of headroom, and each of the two calls that may be in flight has its own); frames beyond that take further trips
 *   of the same workgroups. */
#define PSK_SOFT_VITERBI_SLOTS         16
#define PSK_SOFT_VITERBI_MAX_FRAMES    (1u << 20)
#define PSK_SOFT_VITERBI_MAX_STEPS     65536u
#define PSK_SOFT_VITERBI_SCRATCH_BYTES (256ull << 20)
enum { PSK_SOFT_VITERBI_PACKED = 1, PSK_SOFT_VITERBI_TERMINATED = 2, PSK_SOFT_VITERBI_ANY_START = 4 };  /* psk_soft_viterbi_in_t.flags */
/* psk_soft_viterbi_t.flags: DATA or PLANNED, ORed with the frame's flags shifted left by one */
enum { PSK_SOFT_VITERBI_DATA = 1, PSK_SOFT_VITERBI_REC_PACKED = 2, PSK_SOFT_VITERBI_REC_TERMINATED = 4,
       PSK_SOFT_VITERBI_REC_ANY_START = 8, PSK_SOFT_VITERBI_PLANNED = 128 };

typedef struct psk_soft_viterbi_in {
    const int8_t *llr;    /* DEVICE pointer to the frame's first LLR, any alignment; NULL: the frame is skipped              */
    void *out;            /* DEVICE pointer to the output: n_bits bytes, or ceil(n_bits / 8) with PACKED; any alignment     */
    uint32_t n_steps;     /* trellis steps (input bits including the tail); 0: the frame is skipped                         */
    uint32_t code;        /* 1 + the slot of the code; 0: the frame is skipped                                              */
    uint32_t flags;       /* PSK_SOFT_VITERBI_PACKED, _TERMINATED, _ANY_START                                               */
    uint32_t pad;         /* zero                                                                                           */
} psk_soft_viterbi_in_t;  /* 32 bytes */

typedef struct psk_soft_viterbi {        /* one per frame of the LAST psk_soft_viterbi_device call */
    uint64_t n_steps;
    uint64_t n_llr;                      /* the LLRs read                                                                   */
    int64_t metric;                      /* the end state's path metric, minus nothing                                     */
    int64_t sum_abs;                     /* sum |l| over the LLRs read, with |-128| = 128                                   */
    uint32_t n_flip;                     /* LLRs l != 0 whose sign disagrees with the decoded path's code bit: the channel-
                                            error count a caller uses as a lock indicator                                  */
    uint32_t n_zero;                     /* LLRs equal to 0                                                                 */
    uint32_t end_state, start_state;
    uint32_t n_bits;
    uint32_t flags;                      /* PSK_SOFT_VITERBI_DATA or _PLANNED, | the frame's flags shifted left by one      */
    uint32_t pad[2];                     /* zero                                                                            */
} psk_soft_viterbi_t;                    /* 64 bytes */

/* The code of slot `slot` (0 .. PSK_SOFT_VITERBI_SLOTS - 1), copied into memory the handle owns; a frame names it as code =
 * slot + 1.  Redefining a slot waits for the handle's last viterbi launch first.  A control-plane-only handle records the code.
 * PSK_SOFT_ERR_INVALID_ARG: a null pointer, a slot out of range, K outside 3 .. 7, n outside 2 .. 4, a polynomial the text above
 * refuses, P outside 1 .. 16 or n*P > 32, a keep of 0 or with bits at or above n*P. */
psk_soft_status psk_soft_viterbi_define(psk_soft_handle_t *h, uint32_t slot, uint32_t K, uint32_t n, const uint32_t *g /* [n] */,
                                        uint32_t P, uint32_t keep);
/* The frames in[0 .. nframe-1], nframe = 1 .. PSK_SOFT_VITERBI_MAX_FRAMES.  The LLRs must be complete on `stream` (a demap call
 * enqueued there just before is); with PSK_SOFT_OPT_DEFERRED_JOIN pending the call joins the side streams into `stream` first,
 * as the sync and demap entries do.  The call returns without waiting.  Every call replaces the records.
 * A frame with n_steps == 0, code == 0 or llr == NULL is skipped: it gets the all-zero record and nothing is written.
 * Refusals (PSK_SOFT_ERR_INVALID_ARG before anything is enqueued or any record changes): a null pointer, nframe out of range; on
 * a frame that is not skipped a slot out of range or never defined, unknown flag bits, a non-zero pad, a null `out`, n_steps
 * above PSK_SOFT_VITERBI_MAX_STEPS, TERMINATED with n_steps < K-1.
 * How: one launch on `stream`, one wave per frame (see Cost above); frames beyond 65535 workgroups or beyond the scratch bound
 * take further trips of the same workgroups.
 * A control-plane-only handle checks the arguments, then leaves records with n_steps, n_llr, n_bits and flags =
 * PSK_SOFT_VITERBI_PLANNED | the frame's flags shifted left by one, everything else zero. */
psk_soft_status psk_soft_viterbi_device(psk_soft_handle_t *h, uint32_t nframe, const psk_soft_viterbi_in_t *in /* [nframe] */,
                                        void *stream);
/* waits like psk_soft_get_demap does and copies the records of the frames [first, first + n) of the last call out.
 * PSK_SOFT_ERR_INVALID_ARG: a null pointer, n == 0, a range beyond the last call's nframe, no call yet. */
psk_soft_status psk_soft_get_viterbi(psk_soft_handle_t *h, uint32_t first, uint32_t n, psk_soft_viterbi_t *rec /* [n] */);
/* host only, pure: the definition for one frame on the host.  `in` is read as the entry reads it, with HOST pointers in llr and
 * out; `code` is not looked at beyond being non-zero (the code is K, n, g, P, keep).  The bytes at out and *rec are byte for byte
 * what the device writes (flags = PSK_SOFT_VITERBI_DATA | ...).  A skipped frame gives the zero record.  Refuses what the entry
 * and psk_soft_viterbi_define refuse of their arguments. */
psk_soft_status psk_soft_viterbi_host(uint32_t K, uint32_t n, const uint32_t *g, uint32_t P, uint32_t keep,
                                      const psk_soft_viterbi_in_t *in, psk_soft_viterbi_t *rec);
/* host only, pure: the encoder with puncturing applied, from state 0: bits[0 .. n_steps-1] (uint8, the low bit counts; a caller
 * that terminates appends its K-1 zeros itself) to psk_soft_viterbi_count(...) code bits, one a byte (0 / 1), in order of (t, j). */
psk_soft_status psk_soft_viterbi_encode_host(uint32_t K, uint32_t n, const uint32_t *g, uint32_t P, uint32_t keep, const uint8_t *bits,
                                             uint32_t n_steps, uint8_t *code_bits_out);
/* host only, pure: the number of LLRs a frame of n_steps steps holds; 0 for arguments psk_soft_viterbi_define refuses of n, P, keep
 * (K is not looked at) */
uint64_t psk_soft_viterbi_count(uint32_t K, uint32_t n, uint32_t P, uint32_t keep, uint64_t n_steps);
uint64_t psk_soft_viterbi_bytes(void);      /* sizeof(psk_soft_viterbi_t), for bindings */
uint64_t psk_soft_viterbi_in_bytes(void);   /* sizeof(psk_soft_viterbi_in_t), for bindings */

/* ---- frames as corrected bytes: Reed-Solomon decoding of byte frames ----------------------------------------------------------------
 * The outer code behind the decoder above: the psk_soft_rs_ family -- its definition, structs and seven entries -- is declared in
 * psk_soft_rs.h, which this header includes here, so that one include still declares the whole interface. */
#include "psk_soft_rs.h"

/* ---- frames as aligned bytes: between the decoder and the outer code ----------------------------------------------------------------
 * The psk_soft_frame_ family -- the word search in the decoded bits and the cut of aligned, deinterleaved byte frames -- is declared
 * in psk_soft_frame.h, included here in the same way. */
#include "psk_soft_frame.h"

/* Force every channel through the reference-order (sequential) kernel: 1 on, 0 off. */
psk_soft_status psk_soft_set_force_sequential(psk_soft_handle_t *h, int on);

/* Page-locked host memory that the GPU reads and writes directly (hipHostMalloc): packets and result
 * buffers allocated here can be handed to psk_soft_process_device as they are -- the kernels stream
 * them over PCIe with no staging copy (measured 55 GB/s in + 16 GB/s out, i.e. link rate, against
 * 32 + 9 GB/s for pageable buffers through psk_soft_process_host).  The replacement for the
 * std::vector storage of bulkio dataTransfer::dataBuffer (reference cpp/psk_soft.cpp:349, 428) in a
 * host that wants the link rate.  NULL on failure / without a GPU. */
void *psk_soft_host_alloc(size_t bytes);
void psk_soft_host_free(void *p);

/* Device (HBM) buffers on the handle's GPU for callers that keep packets and results resident and have no HIP
 * runtime of their own to allocate them with (hipMalloc / hipFree / hipMemcpy behind the handle's device; the
 * copies are synchronous).  A host that already owns device memory -- torch tensors, its own hipMalloc --
 * passes those pointers to psk_soft_process_device directly and never needs these. */
void *psk_soft_device_alloc(psk_soft_handle_t *h, size_t bytes);
void psk_soft_device_free(psk_soft_handle_t *h, void *p);
psk_soft_status psk_soft_device_upload(psk_soft_handle_t *h, void *dev_dst, const void *host_src, size_t bytes);
psk_soft_status psk_soft_device_download(psk_soft_handle_t *h, void *host_dst, const void *dev_src, size_t bytes);

/* Measurement support ("the empirical ceiling on the box -- a pure float4
 * read-reduce kernel over the same buffer"): reads `bytes` of device memory at `dev_ptr` (16-byte
 * aligned) `reps` times with 16-byte loads, nothing else, and returns the mean duration of one pass in
 * milliseconds, timed with HIP events on the handle's stream.  No counterpart in the reference. */
psk_soft_status psk_soft_probe_read_ms(psk_soft_handle_t *h, const void *dev_ptr, uint64_t bytes, int reps,
                                       double *ms_per_pass);

/* checkpoint / test support: opaque state blob of one channel */
uint64_t psk_soft_state_bytes(const psk_soft_handle_t *h);
psk_soft_status psk_soft_export_state(psk_soft_handle_t *h, uint32_t ch, void *dst, uint64_t cap);
psk_soft_status psk_soft_import_state(psk_soft_handle_t *h, uint32_t ch, const void *src, uint64_t bytes);
/* introspection of the mirrored control state (tests): samples.size(), index, yvals.size() */
psk_soft_status psk_soft_peek(const psk_soft_handle_t *h, uint32_t ch, uint64_t *ring_len,
                              uint64_t *index, uint64_t *fit_len);

#ifdef __cplusplus
}
#endif
#endif /* PSK_SOFT_HIP_H */
