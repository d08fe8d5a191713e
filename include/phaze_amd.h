/*
 * phaze_amd.h -- C ABI of the MI355X-native phase-vocoder pitch shifter (drop-in boundary).
 *
 * This library replaces ONE path of olvb/phaze: the AudioWorkletProcessor call
 *     process(inputs, outputs, {pitchFactor}) -> true
 * of OLAProcessor.process                (/root/reference/src/ola-processor.js:159-171) with
 *    PhaseVocoderProcessor.processOLA    (/root/reference/src/phase-vocoder.js:45-72) and the fft.js
 *    arithmetic it calls                 (/root/reference/www/phase-vocoder.js:2-508).
 * The reference has no FFI (it is JavaScript in a browser audio thread); the functions below are what a
 * Node.js N-API addon (phaze_amd/node/phaze_napi.c) or any other FFI (ctypes, cgo, JNI) binds.
 * See INTEGRATION.md for the reference-side binding.
 *
 * Conventions: plain C types only; the caller owns every I/O buffer; the library owns all device state;
 * every function returns an int status (PV_OK == 0) and never throws or aborts across the boundary.
 * A handle is NOT thread-safe (the reference runs on one audio thread: one caller per handle).
 */
#ifndef PHAZE_AMD_H
#define PHAZE_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#if defined(__GNUC__)
#define PV_API __attribute__((visibility("default")))
#else
#define PV_API
#endif

/* ---- status codes ---- */
enum {
    PV_OK = 0,
    PV_ERR_FFT_SIZE = 1,     /* 'FFT size must be a power of two and bigger than 1' (bundle:6-7)        */
    PV_ERR_ARGUMENT = 2,     /* NULL pointer, negative count, hop does not divide fft_size, ...          */
    PV_ERR_UNSUPPORTED = 3,  /* valid for the reference but outside this build's kernel range (2..1048576)  */
    PV_ERR_CAPACITY = 4,     /* more channels / hops than the handle was created for                     */
    PV_ERR_DEVICE = 5,       /* HIP runtime error (no GPU, launch failure, out of memory)                */
    PV_ERR_DESTROYED = 6     /* handle already destroyed                                                  */
};

typedef struct pv_handle pv_handle;

/* Version of this header's binary interface (struct layouts + semantics).  pv_abi_version() returns the value the LIBRARY was built with;
 * 2 = round 3: pv_config carries its own size, unknown pv_config.flags bits are rejected, PV_FLAG_PERSISTENT_STREAM;
 * 3 = round 4: pv_host_alloc / pv_host_free (page-locked host buffers: pv_process_batch pipelines them), PV_FLAG_TEST_NO_HDP_FLUSH,
 *     pv_reset_channels_part + PV_FLAG_HOST_CHANNEL_BOOKKEEPING;
 * 4 = round 5: PV_FLAG_FP64_FORWARD, pv_forward_stats;
 * 5 = round 6: PV_FLAG_TEST_FAIL_SECOND_PIECE (a test hook); no layout or semantic change of anything that existed;
 * 6 = the time-stretch handle (pv_stretch_config, pv_stretch_*); nothing that existed changed.  Later, still 6 (additive: new symbols only, no
 *     layout or semantic change): variable tempo on that handle, pv_tempo_process / pv_tempo_process_device; linked channels,
 *     pv_link_channels (an unlinked handle behaves as before); phase resets and onset strength, pv_transient_process / _device,
 *     pv_onset_strength / _device, pv_transient_plan, pv_onsets_from_strength (pv_tempo_process is unchanged); the resampler and pitch handles, pv_resample_*, pv_pitch_*;
 *     the variable-ratio resampler and the pitch-curve handle, pv_vari_*, pv_glide_*; the f0 tracker and the pitch-correction planner, pv_f0_*,
 *     pv_tune_plan; pitch-synchronous overlap-add, pv_psola_*; its epoch marks, pv_epoch_*; its time-scale modification, pv_tsm_*; its harmony voices,
 *     pv_harmony_*; its per-take plans, pv_takes_*; its mirrored grains, pv_mirror_*; its warped grains (formant shifting), pv_formant_*;
 *     pitch contour tracking, pv_contour_*; full-grain harmony voices (mirrored and warped grains in every voice), pv_choir_*. */
#define PV_ABI_VERSION 6

/* Construction options.  Replaces `new PhaseVocoderProcessor(options)` (phase-vocoder.js:24-43,
 * ola-processor.js:7-34).  The reference hard-codes fft_size 2048 (phase-vocoder.js:6) and hop 128
 * (ola-processor.js:3); both are options here; the host layer (phaze_amd/node/phase-vocoder.js) supplies the reference's values when omitted. */
typedef struct pv_config {
    int32_t struct_size;     /* sizeof(pv_config) as the CALLER compiled it (PV_CONFIG_INIT sets it).  pv_create rejects any other value with
                              * PV_ERR_ARGUMENT: a caller built against another layout would otherwise have trailing fields (flags!) read as garbage */
    int32_t fft_size;        /* N, power of two > 1 (else PV_ERR_FFT_SIZE); kernels cover 2..1048576      */
    int32_t hop_size;        /* h >= 2, divides N.  nbOverlaps R = N / h (ola-processor.js:17)           */
    int32_t max_channels;    /* channel slots owned by this handle (streams x channels); 0 => 2.  One launch
                              * takes any count for N = 1024 (hops 128..1024) and up to 65535 otherwise (PV_ERR_CAPACITY) */
    int32_t max_hops;        /* largest nhops of a host-buffer batch call (staging size); 0 => 1        */
    int32_t device_id;       /* HIP device ordinal                                                       */
    int32_t frames_per_chunk;/* batch kernel: output hops per workgroup (0 => auto)                      */
    int32_t flags;           /* PV_FLAG_* bits, 0 for production use                                     */
} pv_config;
/* pv_config cfg = PV_CONFIG_INIT; cfg.fft_size = ...;  (every other field 0 = its default) */
#define PV_CONFIG_INIT { (int32_t)sizeof(pv_config), 0, 0, 0, 0, 0, 0, 0 }

/* pv_config.flags: explicit A/B switches for tests and measurements (the library reads NO environment
 * variables).  All select complete, parity-tested implementations of the same path. */
enum {
    PV_FLAG_GENERIC_KERNEL = 1, /* always launch the LDS-staged fallback kernel (pv_chain_kernel)        */
    PV_FLAG_STREAM_COPY = 2,    /* streaming quantum through H2D + kernel + D2H copies instead of the
                                 * zero-copy mapping of the pinned staging buffer                         */
    PV_FLAG_WORKGROUP_KERNEL = 4, /* N = 2048 / 4096 / 8192: the eight-element workgroup kernel (pv_wg_kernel) instead of the
                                  * one-wave (pv_wave2k_kernel) / sixteen-element (pv_wg16_kernel) kernels */
    PV_FLAG_STREAM_EVENT_WAIT = 8, /* streaming quantum: wait through hipStreamSynchronize (round-2 behaviour).  Default since round 3: every
                                  * frame chain stores a sequence number into pinned host memory when its output is written and pv_process /
                                  * pv_process_end spin on those words (bounded; falls back to the stream wait) -- the runtime's completion
                                  * path costs more than the kernel of a quantum */
    PV_FLAG_STREAM_PINNED_INPUT = 16, /* streaming quantum: the kernel READS its hop from pinned host memory over PCIe (the round-2/3 form).  Default
                                  * since round 3 on a large-BAR device (hipDeviceAttributeIsLargeBar; every MI355X): a quantum of up to 16 KB of input
                                  * is written by the HOST into device memory through the BAR (posted writes, ordered before the launch doorbell),
                                  * so the kernel starts on local HBM instead of a PCIe read round trip; larger quanta and other devices keep the
                                  * pinned-memory read.  The output always goes to pinned host memory (posted device writes) */
    PV_FLAG_PERSISTENT_STREAM = 32, /* streaming quanta on a RESIDENT kernel (N = 1024 and 2048 with the hops their one-wave kernels cover, N = 8192 with
                                  * hop >= N/8; at most 64 channel slots; ignored elsewhere): the kernel of the first pv_process stays on the GPU, one wave
                                  * (N = 8192: one workgroup) per channel slot polling a control word -- in device memory, written by the host through the
                                  * large BAR together with quanta of up to 16 KB of input; in pinned host memory on other devices / with
                                  * PV_FLAG_STREAM_PINNED_INPUT.  A quantum then costs no launch.  The waves leave by themselves after ~50 ms without work
                                  * (and are relaunched on demand) and before any other use of the handle's stream (batch calls, state export / import,
                                  * reset, pv_synchronize).  Same kernel code, same bits as the launch-per-quantum form.  Off by default: while resident, a
                                  * device-wide synchronize of another user of the GPU waits for that idle time-out, and the handle should keep its own
                                  * stream (pv_set_stream to a stream shared with other work would queue that work behind the resident kernel) */
    PV_FLAG_TEST_NO_HDP_FLUSH = 64, /* TEST HOOK, never needed in production: behave as if the device did not expose its HDP flush register
                                  * (hipDeviceAttributeHdpMemFlushCntl).  The library then must not hand quanta over through the BAR -- a host store
                                  * could still sit in the device's host data path when the kernel reads -- and falls back to the pinned-memory
                                  * form on its own; tests/test_gpu_stream_forms.py runs every hand-over form under this bit */
    PV_FLAG_HOST_CHANNEL_BOOKKEEPING = 128, /* pv_process / pv_process_begin do NOT reset the channel state when nch differs from the previous call: the host does the
                                  * reference's bookkeeping itself with pv_reset_channels_part -- input and output buffers separately, ola-processor.js:38-52 -- as
                                  * phaze_amd/node/phase-vocoder.js does for hosts whose outputs do not mirror their inputs */
    PV_FLAG_FP64_FORWARD = 256,  /* every frame's forward transform in fp64, as the reference computes it (realTransform on JS doubles, bundle:306-508) and as every
                                  * round-4 kernel did.  Default since round 5 (N = 1024 and N = 2048): the forward transform runs in packed fp32 FIRST and the peak decisions
                                  * (phase-vocoder.js:95-116) are taken on its magnitudes wherever every comparison they rest on lies outside a guard band around the fp32
                                  * transform's error; a frame with a comparison inside the band re-runs its forward transform in fp64 (pv_forward_stats counts them).
                                  * The band is an EMPIRICALLY VALIDATED law, not an analytic bound: g = 10 eps max|X| against a largest observed discrepancy of 3.3
                                  * (a rigorous FFT error bound in max|X| terms is ~20x wider).  What backs "the decisions are the fp64 transform's" is a validation
                                  * build in which every frame computes both transforms and compares the two sets of peak flags: 0 frames whose flags differ without
                                  * the band asking for the fp64 transform over 4.7e7 + 1.2e7 frames (profiles/r05_flip_count*.json), re-measured on every GPU test run
                                  * over fifteen signal classes incl. four adversarial ones (tests/test_gpu_flip_count.py, >= 2.9e6 frames, band-shrink margin >= 2
                                  * asserted, 4.5 measured).  An uncaught flip would misplace one region of one frame (far inside the 1e-4 RMS bar) -- set this flag where
                                  * decision parity must hold by construction.  The source spectrum of a guarded frame carries the fp32 transform's rounding
                                  * (~1e-7 of the frame's rms instead of a correctly rounded fp64 value).  Which frames fall back depends on their own samples only:
                                  * chunked, call-split, streaming and batch runs of one stream still agree bit for bit */
    PV_FLAG_TEST_FAIL_SECOND_PIECE = 512, /* TEST HOOK, never needed in production: a pipelined host-buffer batch (pv_process_batch on page-locked memory, >= 4 MB) reports
                                  * PV_ERR_DEVICE behind its second piece, as a failed copy or launch would -- tests/test_gpu_batch_pipeline.py checks that the handle is
                                  * rolled back to its state before the call (timeCursor, ping-pong half, the state snapshot of a hop-span pipeline) */
    PV_FLAG_ALL = 1023           /* every bit this build knows: pv_create rejects anything else (PV_ERR_ARGUMENT) */
};

typedef struct pv_info {
    int32_t fft_size, hop_size, overlaps, max_channels, max_hops;
    int32_t threads_per_workgroup, lds_bytes_per_workgroup, frames_per_chunk;
    int32_t compute_units, device_id;
    char device_name[64];
    char kernel_name[32];    /* "pv_wave_kernel_1024" (N = 1024, hop in {128,256,512,1024}), "pv_wave2k_kernel" (N = 2048, hop in
                              * {128,256,512,1024,2048}: one wave per frame), "pv_wg16_kernel" (N = 4096 / 8192, hop in {N/8, N/4, N/2,
                              * N}: two / four waves per frame, sixteen elements per thread), "pv_wg_kernel" (N >= 2048 with smaller even
                              * hops that fit LDS, and PV_FLAG_WORKGROUP_KERNEL: a workgroup per frame, eight elements per thread) or
                              * "pv_chain_kernel" (everything else / PV_FLAG_GENERIC_KERNEL) */
} pv_info;

/* ---- lifetime ---------------------------------------------------------------------------------- */
/* Allocates device state (zeroed input history + overlap-add accumulators, timeCursor = 0) and the
 * FFT/Hann tables.  Replaces the constructor chain phase-vocoder.js:24-43 -> ola-processor.js:7-34.  */
PV_API int pv_create(const pv_config *cfg, pv_handle **out);
/* PV_ABI_VERSION of the loaded library (a binding checks it against the header it was generated from). */
PV_API int pv_abi_version(void);
PV_API int pv_destroy(pv_handle *h);

/* Human-readable text of the last failure on this handle (h == NULL: of the last failed pv_create). */
PV_API const char *pv_last_error(const pv_handle *h);
PV_API const char *pv_status_string(int status);
PV_API int pv_get_info(const pv_handle *h, pv_info *out);
/* Number of HIP devices this process can create handles on (pv_config.device_id in [0, count)): what a host needs to shard streams over the
 * GPUs of a node (stream s -> device s mod count; streams are independent processors, nothing is exchanged). */
PV_API int pv_device_count(int32_t *out);

/* Forward-transform statistics since the handle was created (or last reset): frames whose forward transform an fp32-first kernel instance computed, and how many
 * of them re-ran it in fp64 because a peak decision (phase-vocoder.js:95-116) was within the fp32 transform's error (PV_FLAG_FP64_FORWARD).  Frames that run on
 * instances without the fp32-first path are not counted.  Synchronizes the handle's stream -- and, like every call that puts work on that stream, first asks the resident
 * waves of a PV_FLAG_PERSISTENT_STREAM handle to leave (the next quantum relaunches them: ~20 us once): poll it between streams, not between quanta.  Either pointer may be
 * NULL; reset != 0 zeroes the counters. */
PV_API int pv_forward_stats(pv_handle *h, uint64_t *frames, uint64_t *fallbacks, int32_t reset);

/* ---- state ------------------------------------------------------------------------------------- */
/* Zero history + accumulators of ALL channels and set timeCursor = 0 (a freshly constructed processor). */
PV_API int pv_reset(pv_handle *h);
/* Zero history + accumulator of channel slots [first, first+count): what allocateInputChannels /
 * allocateOutputChannels do when a channel count changes (ola-processor.js:38-52,54-88).  timeCursor kept. */
PV_API int pv_reset_channels(pv_handle *h, int32_t first, int32_t count);
/* The same for ONE side of the state: the reference reallocates inputBuffers when inputs[i].length changes (ola-processor.js:40-44,54-71: the input history
 * restarts from zeros) and outputBuffers when outputs[i].length changes (:46-51,73-88: the pending overlap-add sums restart from zeros) -- two separate
 * events for a host whose outputs do not mirror its inputs.  parts = PV_STATE_HISTORY | PV_STATE_ACCUMULATOR bits. */
enum { PV_STATE_HISTORY = 1, PV_STATE_ACCUMULATOR = 2 };
PV_API int pv_reset_channels_part(pv_handle *h, int32_t first, int32_t count, int32_t parts);
/* timeCursor (phase-vocoder.js:31,71): samples consumed so far = hops * hop_size.  The reference only ever
 * advances it by hop_size (pv:71), so a value that is negative or not a multiple of hop_size is rejected
 * with PV_ERR_ARGUMENT (the register kernels rely on t = m * hop for their exact rotations). */
PV_API int pv_get_time_cursor(const pv_handle *h, int64_t *out);
PV_API int pv_set_time_cursor(pv_handle *h, int64_t value);

/* State export / import of ONE channel slot: everything the reference keeps between process() calls for a channel --
 * hist[N - hop] = the newest N - hop input samples (inputBuffers, ola-processor.js:59,121-127), acc[N - hop] = the pending
 * overlap-add sums (outputBuffers, ola-processor.js:77,130-137) -- plus the processor-wide timeCursor (phase-vocoder.js:31).
 * Checkpoint / resume, moving a stream to another handle or GPU, and splitting ONE stream along the time axis all reduce to
 * this: a handle that imports the state another one exported continues bit for bit.  (Time-sharding needs no hand-over at all:
 * hist is plain input, and the accumulator only depends on the last R - 1 frames, so a span can import {input tail, acc = 0,
 * cursor} R - 1 hops early and recompute its halo; see bench.py --time-shard.)  Synchronous.  hist / acc may be NULL (skipped);
 * pv_import_state sets the handle's timeCursor when time_cursor >= 0 (multiple of hop_size) and leaves it when negative. */
PV_API int pv_export_state(pv_handle *h, int32_t ch, float *hist, float *acc, int64_t *time_cursor);
PV_API int pv_import_state(pv_handle *h, int32_t ch, const float *hist, const float *acc, int64_t time_cursor);

/* ---- the hot call, streaming form (one render quantum) ------------------------------------------- */
/* Replaces OLAProcessor.process(inputs, outputs, parameters) (ola-processor.js:159-171) for ONE input /
 * ONE output with nch channels:  in[c] -> nsamples (== hop_size) host floats, valid only during the call;
 * out[c] <- hop_size floats.  pitch_factor = parameters.pitchFactor[last] (phase-vocoder.js:47).
 * nsamples == 0 (or in == NULL) reproduces the paused branch (ola-processor.js:93-100): the newest hop
 * is treated as zeros, timeCursor still advances.  A change of nch against the previous call resets all
 * channel state first (ola-processor.js:38-52).  Synchronous: outputs are valid on return.  PV_OK <=> the
 * reference's `return true`. */
PV_API int pv_process(pv_handle *h, const float *const *in, float *const *out, int32_t nch,
                      int32_t nsamples, float pitch_factor);

/* The same quantum split into its launch and its wait, for a host that drives SEVERAL handles (the inputs of one processor with
 * numberOfInputs > 1, phase-vocoder.js:49-50, or handles on different GPUs): call pv_process_begin on every handle -- each copies its
 * blocks to pinned memory and launches on its own stream, nothing waits -- then pv_process_end on every handle.  All launches are in
 * flight before the first wait.  pv_process(h, in, out, ...) == pv_process_begin(h, in, ...) + pv_process_end(h, out).  Between the two calls
 * the handle accepts no other call; pv_process_end without a pending quantum returns PV_ERR_ARGUMENT.  When the wait fails the handle is
 * rolled back to its state before pv_process_begin. */
PV_API int pv_process_begin(pv_handle *h, const float *const *in, int32_t nch, int32_t nsamples, float pitch_factor);
PV_API int pv_process_end(pv_handle *h, float *const *out);

/* ---- the hot call, batch (throughput) form ------------------------------------------------------- */
/* nhops consecutive process() calls for nch channel slots in one launch.  Planar layout: channel c
 * occupies in[c*ch_stride .. c*ch_stride + nhops*hop_size), same for out.  pitch[m] is the k-rate
 * pitchFactor of hop m; with pitch_stride != 0 channel c uses the row of its stream,
 * pitch[(c / channels_per_stream) * pitch_stride + m] (independent processors batched together).
 * State (history, accumulator tail, timeCursor) carries across calls exactly as if process() had been
 * called hop by hop.  Host-pointer variant: synchronous, stages through device memory.  When `in` and `out` are page-locked memory
 * (pv_host_alloc below, or anything hipHostMalloc / hipHostRegister produced) a batch of 4 MB or more is PIPELINED: cut into up to 16 pieces
 * -- groups of whole streams when there are enough, else spans of hops -- with piece k+1 on its way to the device while piece k is in the
 * kernel and piece k-1 on its way back (DMA both ways at once; the results are bit-identical to the unpipelined call).  Pageable buffers
 * work as before (the runtime stages them synchronously: several times slower). */
PV_API int pv_process_batch(pv_handle *h, const float *in, float *out, int32_t nch, int32_t nhops,
                            int64_t ch_stride, const float *pitch, int32_t pitch_stride,
                            int32_t channels_per_stream);

/* Page-locked host memory for the batch call above (hipHostMalloc, visible to every device of the process): what a host that owns its audio
 * buffers should put them in -- the N-API addon hands it out as external ArrayBuffers (native.allocPinned), so that a Node host writes its
 * streams in place.  Replaces the `new Float32Array(...)` a caller of OLAProcessor.process owns (ola-processor.js:159-171 receives host
 * arrays).  No handle needed; pv_host_free(NULL) is a no-op. */
PV_API int pv_host_alloc(size_t bytes, void **out);
PV_API int pv_host_free(void *p);

/* Device-pointer variant: in/out/pitch are DEVICE pointers (HBM-resident), the launch is asynchronous on
 * the handle's stream (pv_set_stream / pv_synchronize).  This is the form bench.py times. */
PV_API int pv_process_batch_device(pv_handle *h, const float *d_in, float *d_out, int32_t nch,
                                   int32_t nhops, int64_t ch_stride, const float *d_pitch,
                                   int32_t pitch_stride, int32_t channels_per_stream);

/* Use an externally owned hipStream_t (e.g. torch.cuda.current_stream().cuda_stream); NULL => the
 * handle's own stream. */
PV_API int pv_set_stream(pv_handle *h, void *hip_stream);
PV_API int pv_synchronize(pv_handle *h);

/* ---- test taps ----------------------------------------------------------------------------------- */
/* Runs ONE frame of channel `ch` through the kernels from the CURRENT state without changing it and
 * returns the intermediates the reference keeps in freqComplexBuffer / magnitudes / peakIndexes /
 * freqComplexBufferShifted (phase-vocoder.js:37-42): X[2N] doubles (bins 0..N/2 and, when the frame reads
 * it, the above-Nyquist residue), mag[N/2+1], peak_flags[N/2+1] (0/1), Y[2*(N/2+1)] floats.
 * block: hop_size host floats (the newest hop).  Any output pointer may be NULL. */
PV_API int pv_debug_frame(pv_handle *h, int32_t ch, const float *block, float pitch_factor, double *X,
                          float *mag, int32_t *peak_flags, float *Y);

/* ---- time stretch: tempo change at constant pitch (a separate handle) ----------------------------- */
/* Phase-locked phase vocoder (Laroche-Dolson identity phase locking) on the pitch path's analysis front end: periodic Hann, fp64 forward
 * transform, computeMagnitudes / findPeaks (phase-vocoder.js:82-116) and the region-of-influence rule of shiftPeaks at f = 1 (:131-141).
 * Each frame consumes analysis_hop (ha) input samples and emits synthesis_hop (hs) output samples: the output lasts hs / ha times as long.
 * Phases are u32 fixed-point turns, so every carried quantity is an integer sum: any split of a stream into calls gives the same bits.
 * The output lags the input by N - hs samples.  N = 256 .. 8192 (outside: PV_ERR_FFT_SIZE / PV_ERR_UNSUPPORTED as pv_create), ha in 1..N,
 * hs in 1..N/2 (at least two overlapping output frames; each frame is scaled by hs / N).  See INTEGRATION.md "Time stretch".
 * Each channel slot keeps its own phases unless pv_link_channels groups them (one phase track per group: the stereo image survives). */
typedef struct pv_stretch_config {
    int32_t struct_size;     /* sizeof(pv_stretch_config) as the caller compiled it (PV_STRETCH_CONFIG_INIT sets it)          */
    int32_t fft_size;        /* N, power of two, 256 .. 8192                                                                      */
    int32_t analysis_hop;    /* ha: input samples per frame, 1 .. N                                                              */
    int32_t synthesis_hop;   /* hs: output samples per frame, 1 .. N/2                                                           */
    int32_t max_channels;    /* channel slots (0 => 1)                                                                           */
    int32_t max_frames;      /* host-pointer calls: staging size in frames (0 => 1); longer calls are staged in pieces          */
    int32_t device_id;       /* HIP device ordinal                                                                               */
    int32_t flags;           /* must be 0                                                                                        */
} pv_stretch_config;
#define PV_STRETCH_CONFIG_INIT { (int32_t)sizeof(pv_stretch_config), 0, 0, 0, 0, 0, 0, 0 }

typedef struct pv_stretch pv_stretch;

/* Config errors are returned before any device is touched; failures are readable through pv_stretch_last_error(NULL). */
PV_API int pv_stretch_create(const pv_stretch_config *cfg, pv_stretch **out);
PV_API int pv_stretch_destroy(pv_stretch *h);
/* Zero the state of every channel slot (a freshly created handle). */
PV_API int pv_stretch_reset(pv_stretch *h);
/* Text of the last failure on this handle (h == NULL: of the last failed pv_stretch_create on this thread). */
PV_API const char *pv_stretch_last_error(const pv_stretch *h);
/* nframes frames for channel slots 0 .. nch-1: in[c*in_stride .. + nframes*ha) -> out[c*out_stride .. + nframes*hs).
 * Host pointers, synchronous. */
PV_API int pv_stretch_process(pv_stretch *h, const float *in, float *out, int32_t nch, int32_t nframes,
                              int64_t in_stride, int64_t out_stride);
/* The same on DEVICE pointers, asynchronous on the handle's stream (pv_stretch_set_stream / pv_stretch_synchronize). */
PV_API int pv_stretch_process_device(pv_stretch *h, const float *d_in, float *d_out, int32_t nch,
                                     int32_t nframes, int64_t in_stride, int64_t out_stride);
/* Use an externally owned hipStream_t; NULL => the handle's own stream. */
PV_API int pv_stretch_set_stream(pv_stretch *h, void *hip_stream);
PV_API int pv_stretch_synchronize(pv_stretch *h);
/* State of ONE channel slot: hist[N - ha] newest input samples, acc[N - hs] pending overlap-add sums, phi[N/2 + 1] previous analysis phase,
 * psi[N/2 + 1] synthesis phase (u32 turns).  A handle that imports what another exported continues bit for bit.  Synchronous; any pointer may be
 * NULL (skipped). */
PV_API int pv_stretch_export_state(pv_stretch *h, int32_t ch, float *hist, float *acc, uint32_t *phi, uint32_t *psi);
PV_API int pv_stretch_import_state(pv_stretch *h, int32_t ch, const float *hist, const float *acc,
                                   const uint32_t *phi, const uint32_t *psi);

/* ---- variable tempo on a time-stretch handle: a per-frame analysis hop ------------------------------------------------------------- */
/* Frame m of channel slot c consumes hops[c * hop_stride + m] input samples (hop_stride == 0: every channel uses row 0) and emits synthesis_hop
 * output samples; its window is the newest N samples of the stream, and its hop takes the place of analysis_hop in the phase advance.  The
 * handle's analysis_hop is the FLOOR: every hop must lie in [analysis_hop, N] (the state keeps N - analysis_hop samples of history, all a hop
 * >= the floor needs; create the handle with analysis_hop = 1 for the widest range).  Channel c reads in[c*in_stride .. + sum of its row) and
 * writes out[c*out_stride .. + nframes*hs).  pv_stretch_process is this call with every hop equal to the floor: the two may be mixed on one handle,
 * and any split of a schedule into calls gives the same bits.
 * `hops` is a HOST array in both forms, read before the call returns (it may be reused at once, also after the asynchronous device form).
 * Rejected with PV_ERR_ARGUMENT before any device work, processing nothing and leaving the state untouched: a null buffer, negative counts, a null
 * hops with nframes > 0, a hop_stride that is neither 0 nor >= nframes, a hop outside [analysis_hop, N] (the message names its channel and frame),
 * and with nch > 1 an in_stride below the largest row total or an out_stride below nframes*hs.  nch > max_channels: PV_ERR_CAPACITY.
 * Host pointers, synchronous: staged in pieces of at most max_frames frames (and what fits the input staging, grown once to one frame of hop N). */
PV_API int pv_tempo_process(pv_stretch *h, const float *in, float *out, int32_t nch, int32_t nframes, const int32_t *hops,
                            int64_t hop_stride, int64_t in_stride, int64_t out_stride);
/* The same on DEVICE in / out pointers, asynchronous on the handle's stream. */
PV_API int pv_tempo_process_device(pv_stretch *h, const float *d_in, float *d_out, int32_t nch, int32_t nframes,
                                   const int32_t *hops, int64_t hop_stride, int64_t in_stride, int64_t out_stride);

/* ---- linked channels on a time-stretch handle: one phase track per group ----------------------------------------------------------- */
/* Slots [g*G, (g+1)*G) become group g (G = channels_per_group, 1 .. max_channels; 1 = every slot on its own, the default).  Per frame the group's
 * channels are summed in slot order (f32), that mix runs the phase path of a mono handle (peaks, regions, analysis phase, phase advance), and every
 * channel's bin k is rotated by the mix's angle for k: inter-channel phase and amplitude ratios are kept, and the sum of a group's outputs is the
 * mono stretch of its mix up to rounding.  A frame whose mix has no peak (e.g. an exactly anti-phase pair, L = -R) is silent in every channel.
 * Resets every slot as pv_stretch_reset does (which keeps the setting).  On a linked handle pv_stretch_process* and pv_tempo_process* reject, with
 * PV_ERR_ARGUMENT before any device work and the state untouched, an nch that is not a multiple of G and, with hop_stride != 0, schedule rows that
 * differ within a group (the message names the group and the first frame).  State: the group's phi / psi are read from slot g*G and every call
 * writes them into every slot of the group (export any slot; import into slot g*G); hist / acc stay per slot.  See INTEGRATION.md "Linked channels". */
PV_API int pv_link_channels(pv_stretch *h, int32_t channels_per_group);

/* ---- phase resets on a time-stretch handle: transients pass unstretched ------------------------------------------------------------ */
/* pv_tempo_process plus a HOST row of per-frame flags, resets[c * reset_stride + m] in {0, 1} (reset_stride == 0: every channel uses row 0; else
 * >= nframes, one row per channel slot): a flagged frame sets its synthesis phase to its analysis phase in every bin, psi := q, instead of advancing
 * it, so its rotation angle is zero and its output is Hann * IDFT(X) * hs / N.  Every following frame with hop == synthesis_hop keeps psi == q exactly
 * (integer arithmetic), so a reset followed by a run of unit-tempo frames reproduces the input sample for sample under the overlap-add envelope:
 * the classical way to carry an attack through a stretch.  A reset alone, without the hold, gains nothing (see INTEGRATION.md "Transients").
 * hops == NULL: every hop equals analysis_hop (the fixed-hop call with resets).  resets == NULL: no reset, the bits of pv_tempo_process.  Any split
 * of a schedule into calls gives the same bits, as before; the two rows are HOST arrays read before the call returns.
 * Rejected as pv_tempo_process rejects, and also (PV_ERR_ARGUMENT, before any device work, state untouched): a flag other than 0 / 1, a reset_stride
 * that is neither 0 nor >= nframes, and on a linked handle reset rows that differ within a group (a group has one phase track: psi_g := q of the mix).
 * Host pointers, synchronous, staged in pieces as pv_tempo_process. */
PV_API int pv_transient_process(pv_stretch *h, const float *in, float *out, int32_t nch, int32_t nframes, const int32_t *hops,
                                int64_t hop_stride, const uint8_t *resets, int64_t reset_stride, int64_t in_stride, int64_t out_stride);
/* The same on DEVICE in / out pointers, asynchronous on the handle's stream. */
PV_API int pv_transient_process_device(pv_stretch *h, const float *d_in, float *d_out, int32_t nch, int32_t nframes,
                                       const int32_t *hops, int64_t hop_stride, const uint8_t *resets, int64_t reset_stride,
                                       int64_t in_stride, int64_t out_stride);
/* Onset strength of a buffer, with the stretch's own front end (Hann, fp64 forward, f32 |X|^2; a linked group analyses its f32 mix).  Frames at the
 * handle's analysis_hop: frame m's window is the N samples that end at (m + 1) * analysis_hop, samples before the buffer are zeros, frame -1 is all
 * zeros.  counts[g * count_stride + m] = the number of bins k in [1, N/2) with mag_m[k] > 4 * mag_{m-1}[k] and mag_m[k] > 2^-20 * max_k mag_m, for
 * group g (slot g when unlinked) of in[c * in_stride .. + nframes * analysis_hop).  A pure function of the buffer: it neither reads nor writes the
 * handle's carried state.  A stream analysed in pieces overlaps them by N + analysis_hop samples and drops the frames that saw the padding.
 * Non-finite input: a comparison with a NaN or between two infinities is false, so counts is 0 on every frame whose window holds a NaN or +-Inf
 * sample and on the first frame after those (its previous magnitudes are not finite); every other frame is untouched.
 * Thresholds and peak picking stay with the caller (pv_onsets_from_strength).  Host pointers, synchronous. */
PV_API int pv_onset_strength(pv_stretch *h, const float *in, int32_t nch, int32_t nframes, int64_t in_stride, int32_t *counts,
                             int64_t count_stride);
/* The same on DEVICE in / counts pointers, asynchronous on the handle's stream. */
PV_API int pv_onset_strength_device(pv_stretch *h, const float *d_in, int32_t nch, int32_t nframes, int64_t in_stride,
                                    int32_t *d_counts, int64_t count_stride);
/* Pure host code, no handle and no device.  Frame m is an onset when counts[m] >= tau * (N/2 - 1) and counts[m - 1] is below it (counts[-1] = 0);
 * its position is m * analysis_hop input samples.  tau > 0; 0.4 separates the measured classes (stationary noise <= 0.20, onsets >= 0.66).
 * Two-call sizing, here and in pv_transient_plan: the return value is the number of entries the result has; at most `capacity` of them are written
 * (capacity 0 with NULL arrays only counts).  Errors return -PV_ERR_ARGUMENT. */
PV_API int64_t pv_onsets_from_strength(const int32_t *counts, int64_t nframes, int32_t fft_size, int32_t analysis_hop, double tau,
                                       int64_t *onsets, int64_t capacity);
/* The hop row and reset row of pv_transient_process for sorted onset positions (input samples) in an input of input_len samples: nominal tempo
 * synthesis_hop / nominal_hop, with every onset carried through a hold.  Frame by frame, S the input consumed so far: a frame is HELD when, after
 * its hop, the part [lead, N - lead) of its window meets an attack, taken to last from its onset position to `release` samples behind it (the hop
 * tried is nominal_hop, or synthesis_hop when the previous frame was held);
 * a held frame has hop synthesis_hop, and the first frame of a run of held frames has its reset flag set.  Other frames have hop
 * nominal_hop - clamp(debt, -kappa, kappa) clamped to [floor_hop, N], debt = S - frames * nominal_hop, kappa = max(1, nominal_hop / 8): the total
 * length returns to nominal after each hold.  Stops when the next hop would pass input_len.  floor_hop is the handle's analysis_hop; lead in
 * 0 .. N/2, negative = the default N/8 (N/4 holds too little: measured).  release in 0 .. N, negative = the default N/2; 0 holds only while the
 * onset position itself is inside [lead, N - lead), which ends the hold while the attack's decay is still in the window: the frames after the hold
 * then place that decay late (measured: the attack's energy spread doubles at synthesis_hop = 3N/8).  A hold must in any case exceed N /
 * synthesis_hop frames, release > 2 * lead, for any output to come from held frames alone.  -PV_ERR_ARGUMENT: synthesis_hop < floor_hop (a hold needs hop ==
 * synthesis_hop to be legal: create a speed-up handle with analysis_hop <= synthesis_hop), nominal_hop outside [floor_hop, N], unsorted onsets. */
PV_API int64_t pv_transient_plan(const int64_t *onsets, int64_t nonsets, int64_t input_len, int32_t fft_size, int32_t nominal_hop,
                                 int32_t floor_hop, int32_t synthesis_hop, int32_t lead, int32_t release, int32_t *hops, uint8_t *resets,
                                 int64_t capacity);
/* TEST HOOK, never needed in production: how this chip cuts a call of nch channels and nframes frames into chains (frames per chain; halo =
 * (N - 1) / synthesis_hop earlier frames each chain recomputes), so that tests can put resets on chain and halo boundaries. */
PV_API int pv_transient_chain_layout(pv_stretch *h, int32_t nch, int32_t nframes, int32_t *frames_per_chain, int32_t *halo);
/* TEST HOOK, never needed in production: the frames per chain of a pv_onset_strength call of nch channels and nframes frames on this chip (an onset
 * chain has no halo: it transforms one frame before its own), so that tests can make a chain longer than the kernel's count batch. */
PV_API int pv_onset_chain_layout(pv_stretch *h, int32_t nch, int32_t nframes, int32_t *frames_per_chain);

/* ---- band-limited resampling (a separate handle) ------------------------------------------------------------------------------------- */
/* Polyphase Kaiser-windowed sinc at a rational ratio up / down (output samples per input sample), reduced to L / M by the gcd: 1 <= L, M <= 8192 and
 * 1/8 <= L / M <= 8, anything else PV_ERR_ARGUMENT.  With s = max(1, M / L): half width W = ceil(32 s) input samples, T = 2 W taps per phase, cutoff
 * 0.91 / s of the input Nyquist, Kaiser beta 9; every phase row is divided by its fp64 sum (DC gain 1 in every phase) and rounded once to f32.
 * Output j, counted from the start of the stream, sits at input position j M / L = n_j + phase_j / L and is
 *     y[j] = sum_{i < T} h[phase_j][i] x[n_j - W + 1 + i],   x zero before the stream,
 * accumulated in f32 in the order i = 0, 1, .. T - 1 with one fused multiply-add per tap, whatever the tiling.  After I input samples in total exactly
 * J(I) = max(0, ceil((I - W) L / M)) outputs exist: a call that takes the total from I0 to I1 writes J(I1) - J(I0) samples per channel, all channel slots
 * of a handle move together, the output lags by W input samples, and W zeros drain the stream.  The carried state is the newest T - 1 input samples per
 * slot and the int64 pair (I, J): copies of input and integers, so any split of a stream into calls gives the same bits.  Non-finite input: every
 * output runs all T taps of its phase row, a tap that is 0 included (0 * NaN is NaN), so output j is NaN or +-Inf exactly when one of the T samples
 * x[n_j - W + 1 .. n_j + W] is -- unlike pv_vari, whose zero-weight taps read nothing.  T - 1 clean samples flush the history.  Replaces what the reference
 * leaves to the browser's player (playbackRate, /root/reference/src/main.js:75-96).  See INTEGRATION.md "Pitch". */
typedef struct pv_resample_config {
    int32_t struct_size;     /* sizeof(pv_resample_config) as the caller compiled it (PV_RESAMPLE_CONFIG_INIT sets it)           */
    int32_t up, down;        /* the ratio: up output samples per down input samples                                              */
    int32_t max_channels;    /* channel slots (0 => 1)                                                                           */
    int32_t max_samples;     /* host-pointer calls: staging size in input samples (0 => 4096); longer calls are staged in pieces */
    int32_t device_id;       /* HIP device ordinal                                                                               */
    int32_t flags;           /* must be 0                                                                                        */
} pv_resample_config;
#define PV_RESAMPLE_CONFIG_INIT { (int32_t)sizeof(pv_resample_config), 0, 0, 0, 0, 0, 0 }

typedef struct pv_resample pv_resample;

/* Config errors are returned before any device is touched; failures are readable through pv_resample_last_error(NULL). */
PV_API int pv_resample_create(const pv_resample_config *cfg, pv_resample **out);
PV_API int pv_resample_destroy(pv_resample *h);
/* Zero every slot's history and (I, J): a freshly created handle. */
PV_API int pv_resample_reset(pv_resample *h);
PV_API const char *pv_resample_last_error(const pv_resample *h);
/* Use an externally owned hipStream_t; NULL => the handle's own stream. */
PV_API int pv_resample_set_stream(pv_resample *h, void *hip_stream);
PV_API int pv_resample_synchronize(pv_resample *h);
/* nin new input samples for channel slots 0 .. nch-1, in[c*in_stride .. + nin), write *nout = J(I + nin) - J(I) samples per channel to
 * out[c*out_stride ..) (nout may be NULL).  out_capacity is the room per channel: below what the call produces it is PV_ERR_ARGUMENT before any device
 * work, with the state untouched (so are a null buffer, negative counts and, with nch > 1, strides below nin / the samples produced).  A call shorter
 * than the filter may produce nothing; its input is still carried.  Host pointers, synchronous, staged in pieces of max_samples. */
PV_API int pv_resample_process(pv_resample *h, const float *in, int32_t nch, int64_t nin, int64_t in_stride, float *out, int64_t out_stride,
                               int64_t out_capacity, int64_t *nout);
/* The same on DEVICE in / out pointers, asynchronous on the handle's stream (*nout is known, and written, before the call returns). */
PV_API int pv_resample_process_device(pv_resample *h, const float *d_in, int32_t nch, int64_t nin, int64_t in_stride, float *d_out, int64_t out_stride,
                                      int64_t out_capacity, int64_t *nout);
/* What the next call of nin samples will write per channel. */
PV_API int pv_resample_out_count(const pv_resample *h, int64_t nin, int64_t *nout);
/* State of ONE channel slot, hist[T - 1] = its newest input samples (oldest first), and the handle's pair (I, J).  A handle that imports what another
 * exported continues bit for bit.  Synchronous; any pointer may be NULL (skipped).  pv_resample_import_state sets (I, J) when total_in >= 0 (total_out
 * must then be pv_resample_count of it: PV_ERR_ARGUMENT otherwise) and leaves the pair when total_in is negative. */
PV_API int pv_resample_export_state(pv_resample *h, int32_t ch, float *hist, int64_t *total_in, int64_t *total_out);
PV_API int pv_resample_import_state(pv_resample *h, int32_t ch, const float *hist, int64_t total_in, int64_t total_out);
/* Pure host code, no handle and no device, with the two-call sizing of pv_transient_plan.  pv_resample_design: the table the kernels use, taps[phase * T + i]
 * for phase in [0, L), and the reduced ratio and half width through L, M, W (each may be NULL); returns L * T.  pv_resample_count: J(total_in).
 * Errors return -PV_ERR_ARGUMENT. */
PV_API int64_t pv_resample_design(int32_t up, int32_t down, float *taps, int64_t capacity, int32_t *L, int32_t *M, int32_t *W);
PV_API int64_t pv_resample_count(int32_t up, int32_t down, int64_t total_in);

/* ---- pitch through the stretch: a time-stretch handle followed by a resampler --------------------------------------------------------- */
/* The stretch lengthens the signal by hs / ha at constant pitch; the resampler at up / down then scales duration by up / down and pitch by down / up.
 * Pitch factor down / up, duration factor (hs / ha) (up / down); up = down = 0 means analysis_hop / synthesis_hop: constant duration, pitch x hs / ha,
 * with the stretch's phase locking, linked channels and phase resets.  The handle owns one pv_stretch and one pv_resample and drives them through
 * pv_transient_process_device and pv_resample_process_device on one stream; the stretched signal stays in device memory.  The output lags the input by
 * ((N - hs) + W) L / M output samples.  Replaces the two controls of the reference's application, speed and pitch (/root/reference/src/main.js:75-96). */
typedef struct pv_pitch_config {
    int32_t struct_size;     /* sizeof(pv_pitch_config) as the caller compiled it (PV_PITCH_CONFIG_INIT sets it)                  */
    int32_t fft_size;        /* as pv_stretch_config                                                                             */
    int32_t analysis_hop;    /* ha, the floor of a hop schedule                                                                  */
    int32_t synthesis_hop;   /* hs                                                                                               */
    int32_t up, down;        /* the resampler's ratio; 0 / 0 => analysis_hop / synthesis_hop                                     */
    int32_t max_channels;    /* channel slots (0 => 1)                                                                           */
    int32_t max_frames;      /* frames per call the device buffers are sized for at creation (0 => 1); they grow on demand       */
    int32_t device_id;       /* HIP device ordinal                                                                               */
    int32_t flags;           /* must be 0                                                                                        */
} pv_pitch_config;
#define PV_PITCH_CONFIG_INIT { (int32_t)sizeof(pv_pitch_config), 0, 0, 0, 0, 0, 0, 0, 0, 0 }

typedef struct pv_pitch pv_pitch;

/* Config errors (the stretch's and the resampler's) are returned before any device is touched; readable through pv_pitch_last_error(NULL). */
PV_API int pv_pitch_create(const pv_pitch_config *cfg, pv_pitch **out);
PV_API int pv_pitch_destroy(pv_pitch *h);
PV_API int pv_pitch_reset(pv_pitch *h);
PV_API const char *pv_pitch_last_error(const pv_pitch *h);
/* Both inner handles follow: they always share one stream. */
PV_API int pv_pitch_set_stream(pv_pitch *h, void *hip_stream);
PV_API int pv_pitch_synchronize(pv_pitch *h);
/* nframes frames of pv_transient_process (hops / resets NULL mean what they mean there), resampled: *nout = J(I + nframes * hs) - J(I) samples per channel
 * go to out[c*out_stride ..).  out_capacity below that is PV_ERR_ARGUMENT before any device work with both states untouched, as is everything
 * pv_transient_process rejects.  Host pointers, synchronous. */
PV_API int pv_pitch_process(pv_pitch *h, const float *in, float *out, int32_t nch, int32_t nframes, const int32_t *hops, int64_t hop_stride,
                            const uint8_t *resets, int64_t reset_stride, int64_t in_stride, int64_t out_stride, int64_t out_capacity, int64_t *nout);
/* The same on DEVICE in / out pointers, asynchronous on the handle's stream. */
PV_API int pv_pitch_process_device(pv_pitch *h, const float *d_in, float *d_out, int32_t nch, int32_t nframes, const int32_t *hops, int64_t hop_stride,
                                   const uint8_t *resets, int64_t reset_stride, int64_t in_stride, int64_t out_stride, int64_t out_capacity,
                                   int64_t *nout);
/* The inner handles (owned by h, NULL for a dead handle): pv_link_channels, state export / import and pv_resample_out_count work through them.  Do not
 * destroy them, give them another stream, or process through them directly. */
PV_API pv_stretch *pv_pitch_stretch(pv_pitch *h);
PV_API pv_resample *pv_pitch_resampler(pv_pitch *h);

/* ---- variable-ratio band-limited resampling (a separate handle) ------------------------------------------------------------------------ */
/* The stream moves in blocks of B = block input samples; block b emits counts[b] output samples, min_count <= counts[b] <= max_count, so the local
 * step B / counts[b] (input samples per output sample: the pitch factor) changes from block to block.  1 <= B <= 4096, 1 <= min_count <= max_count
 * <= 8192, B <= 8 min_count and max_count <= 8 B (the step stays within [1/8, 8]); anything else PV_ERR_ARGUMENT.  Half width W = ceil(32 max(1, B /
 * min_count)) <= 256 input samples, T = 2 W.  Output k of stream block b with count c sits at input position b B + k B / c - W: with n = b B + (k B) div c
 * and r = (k B) mod c, tap i = 0 .. T - 1 reads x[n - 2 W + 1 + i] (x zero before the stream) at distance a = |(i - W + 1) c - r| / c from it.  One
 * prototype serves every ratio: P[q] = f32(h0(q / 256)), h0(t) = 0.91 sinc(0.91 t) I0(9 sqrt(1 - (t / 32)^2)) / I0(9), P = 0 from q = 32 * 256 on
 * (pv_vari_prototype).  With den = max(B, c) (the filter widens by max(1, B / c) where a block decimates), in exact integers q = (256 a) div den and
 * rem = (256 a) mod den; the weight is w_i = P[q] + (rem / den) (P[q + 1] - P[q]), 0 when q >= 32 * 256, and
 *     y = (sum_i w_i x_i) / (sum_i w_i),
 * both sums in f32 with i ascending (one fused multiply-add and one add per tap), then one f32 division: unit DC gain at every position and ratio,
 * and the same bits whatever the tiling.  The output lags by W input samples; every output of a block is computable once the block is in, so a call
 * of nblocks blocks consumes nblocks * B samples per channel and writes sum(counts).  The carried state is the newest T - 1 input samples per slot;
 * the int64 counters (blocks, outputs) are informational.  All channel slots of a handle move together.  See INTEGRATION.md "Pitch curves".
 * Non-finite input: a tap whose weight is exactly 0 leaves the sums as they are whatever its sample holds, so output j is NaN or +-Inf exactly when a
 * NaN or +-Inf input sample, carried history included, lies under a tap of j with w_i != 0 (within 32 max(1, B / c) samples of its position); every
 * other output has the value it would have with those samples replaced by 0, in every split of the stream into calls.  The history carries the samples
 * as they came: T - 1 clean samples flush it. */
typedef struct pv_vari_config {
    int32_t struct_size;     /* sizeof(pv_vari_config) as the caller compiled it (PV_VARI_CONFIG_INIT sets it)                   */
    int32_t block;           /* B, input samples per block                                                                       */
    int32_t min_count;       /* the smallest count a call may pass                                                               */
    int32_t max_count;       /* the largest                                                                                      */
    int32_t max_channels;    /* channel slots (0 => 1)                                                                           */
    int32_t max_blocks;      /* host-pointer calls: staging size in blocks (0 => about 4096 samples); longer calls go in pieces  */
    int32_t device_id;       /* HIP device ordinal                                                                               */
    int32_t flags;           /* must be 0                                                                                        */
} pv_vari_config;
#define PV_VARI_CONFIG_INIT { (int32_t)sizeof(pv_vari_config), 0, 0, 0, 0, 0, 0, 0 }

typedef struct pv_vari pv_vari;

/* Config errors are returned before any device is touched; failures are readable through pv_vari_last_error(NULL). */
PV_API int pv_vari_create(const pv_vari_config *cfg, pv_vari **out);
PV_API int pv_vari_destroy(pv_vari *h);
/* Zero every slot's history and the counters: a freshly created handle. */
PV_API int pv_vari_reset(pv_vari *h);
PV_API const char *pv_vari_last_error(const pv_vari *h);
/* Use an externally owned hipStream_t; NULL => the handle's own stream. */
PV_API int pv_vari_set_stream(pv_vari *h, void *hip_stream);
PV_API int pv_vari_synchronize(pv_vari *h);
/* nblocks blocks for channel slots 0 .. nch-1: read in[c*in_stride .. + nblocks*B), write *nout = sum(counts) samples per channel to
 * out[c*out_stride ..) (nout may be NULL; it is written before the call returns).  `counts` is a HOST array in both forms, read before the call
 * returns.  Rejected with PV_ERR_ARGUMENT before any device work, with the state untouched: a null buffer or null counts, negative numbers, a count
 * outside [min_count, max_count] (the message names the block), out_capacity below sum(counts) and, with nch > 1, strides below nblocks*B / sum(counts).
 * nch > max_channels: PV_ERR_CAPACITY.  Host pointers, synchronous, staged in pieces of max_blocks. */
PV_API int pv_vari_process(pv_vari *h, const float *in, int32_t nch, int64_t nblocks, const int32_t *counts, int64_t in_stride, float *out,
                           int64_t out_stride, int64_t out_capacity, int64_t *nout);
/* The same on DEVICE in / out pointers, asynchronous on the handle's stream. */
PV_API int pv_vari_process_device(pv_vari *h, const float *d_in, int32_t nch, int64_t nblocks, const int32_t *counts, int64_t in_stride, float *d_out,
                                  int64_t out_stride, int64_t out_capacity, int64_t *nout);
/* State of ONE channel slot, hist[T - 1] = its newest input samples (oldest first), and the handle's counters (blocks consumed, outputs produced).  A
 * handle that imports what another exported continues bit for bit.  Synchronous; any pointer may be NULL (skipped); pv_vari_import_state leaves the
 * counters when total_blocks is negative. */
PV_API int pv_vari_export_state(pv_vari *h, int32_t ch, float *hist, int64_t *total_blocks, int64_t *total_out);
PV_API int pv_vari_import_state(pv_vari *h, int32_t ch, const float *hist, int64_t total_blocks, int64_t total_out);
/* Pure host code, no handle and no device.  pv_vari_prototype: the table P the kernel uses, 32 * 256 + 2 = 8194 floats with its guard entries, with
 * the two-call sizing of pv_transient_plan (returns 8194, writes at most `capacity`).  pv_vari_half_width: W of a config, or -PV_ERR_ARGUMENT with the
 * reason in pv_vari_last_error(NULL). */
PV_API int64_t pv_vari_prototype(float *table, int64_t capacity);
PV_API int32_t pv_vari_half_width(int32_t block, int32_t min_count, int32_t max_count);

/* ---- pitch curves through the stretch: a time-stretch handle followed by a variable-ratio resampler ------------------------------------- */
/* Frame m consumes hops[m] input samples; the stretch emits synthesis_hop samples for it at constant pitch and the resampler turns that block back
 * into hops[m] samples: duration is kept sample for sample and frame m is shifted in pitch by synthesis_hop / hops[m], with the stretch's phase
 * locking, linked channels and phase resets.  The handle owns one pv_stretch (analysis_hop = min_hop, the floor of every schedule) and one pv_vari
 * (block = synthesis_hop, counts within [min_hop, max_hop]) and drives them through pv_transient_process_device and pv_vari_process_device on one
 * stream; the stretched signal stays in device memory.  min_hop <= hops[m] <= max_hop <= fft_size, synthesis_hop <= 8 min_hop and max_hop <= 8
 * synthesis_hop.  The content lags by (fft_size - synthesis_hop) + W samples of the stretched signal, and the curve acts at output time: a caller
 * shifts the curve by that lag.  tempo_hops(1 / pitch, ...) of the bindings turns a pitch curve into the hop row.  Replaces the pitch fader of the
 * reference's application (/root/reference/src/main.js:75-96). */
typedef struct pv_glide_config {
    int32_t struct_size;     /* sizeof(pv_glide_config) as the caller compiled it (PV_GLIDE_CONFIG_INIT sets it)                  */
    int32_t fft_size;        /* as pv_stretch_config                                                                             */
    int32_t synthesis_hop;   /* hs: the stretch's output per frame, the resampler's block                                        */
    int32_t min_hop;         /* the smallest hop a call may pass (highest pitch: hs / min_hop)                                   */
    int32_t max_hop;         /* the largest (lowest pitch: hs / max_hop)                                                         */
    int32_t max_channels;    /* channel slots (0 => 1)                                                                           */
    int32_t max_frames;      /* frames per call the device buffers are sized for at creation (0 => 1); they grow on demand       */
    int32_t device_id;       /* HIP device ordinal                                                                               */
    int32_t flags;           /* must be 0                                                                                        */
} pv_glide_config;
#define PV_GLIDE_CONFIG_INIT { (int32_t)sizeof(pv_glide_config), 0, 0, 0, 0, 0, 0, 0, 0 }

typedef struct pv_glide pv_glide;

/* Config errors (the stretch's, the resampler's, and max_hop > fft_size) are returned before any device is touched; pv_glide_last_error(NULL). */
PV_API int pv_glide_create(const pv_glide_config *cfg, pv_glide **out);
PV_API int pv_glide_destroy(pv_glide *h);
PV_API int pv_glide_reset(pv_glide *h);
PV_API const char *pv_glide_last_error(const pv_glide *h);
/* Both inner handles follow: they always share one stream. */
PV_API int pv_glide_set_stream(pv_glide *h, void *hip_stream);
PV_API int pv_glide_synchronize(pv_glide *h);
/* nframes frames on ONE HOST row of hops for all channels (required when nframes > 0): channel c reads in[c*in_stride .. + sum(hops)) and writes
 * out[c*out_stride .. + sum(hops)).  resets: as pv_transient_process (NULL: none).  Everything pv_transient_process rejects is rejected here, and a hop
 * outside [min_hop, max_hop], with PV_ERR_ARGUMENT before any device work and both states untouched.  Host pointers, synchronous. */
PV_API int pv_glide_process(pv_glide *h, const float *in, float *out, int32_t nch, int32_t nframes, const int32_t *hops, const uint8_t *resets,
                            int64_t reset_stride, int64_t in_stride, int64_t out_stride);
/* The same on DEVICE in / out pointers, asynchronous on the handle's stream. */
PV_API int pv_glide_process_device(pv_glide *h, const float *d_in, float *d_out, int32_t nch, int32_t nframes, const int32_t *hops,
                                   const uint8_t *resets, int64_t reset_stride, int64_t in_stride, int64_t out_stride);
/* The inner handles (owned by h, NULL for a dead handle): pv_link_channels and state export / import work through them.  Do not destroy them, give
 * them another stream, or process through them directly. */
PV_API pv_stretch *pv_glide_stretch(pv_glide *h);
PV_API pv_vari *pv_glide_resampler(pv_glide *h);

/* ---- pitch tracking and pitch correction: an f0 tracker (a separate handle) and the planner of glide rows ------------------------------- */
/* YIN on block-scaled integers: every value of a record is an exact integer function of the frame's samples, whatever the tiling.  Per channel,
 * frame m reads the W + max_lag samples x[m hop, m hop + W + max_lag) and nothing else: no padding, no carried state; a stream analysed in pieces
 * overlaps them by W + max_lag - hop samples.  16 <= W <= 4096, 2 <= min_lag < max_lag <= 4096, 1 <= hop <= 4096.
 *   scale    A = max |x_i| in f32; a non-finite sample or A == 0 gives the record {0, 0, 0, 0}.  Else A = f 2^e with f in [0.5, 1) and
 *            q_i = rint(x_i 2^(11 - e)), exactly scaled, ties to even: |q_i| <= 2048.
 *   d(tau)   = sum_{i < W} (q_i - q_{i+tau})^2 for tau = 1 .. max_lag (<= 2^36).
 *   c(tau)   = (d(tau) tau 2^14) div cum(tau) in int64, cum(tau) = d(1) + .. + d(tau); 2^14 where cum(tau) == 0, and c(0) = 2^14.
 *   pick     the smallest tau in [min_lag, max_lag - 1] with c(tau) < threshold, advanced while tau < max_lag - 1 and c(tau + 1) < c(tau): the record
 *            is {tau, c(tau - 1), c(tau), c(tau + 1)}.  No such tau: the frame is unvoiced, b is the first argmin of c over [min_lag, max_lag - 1] and
 *            the record is {-b, c(b - 1), c(b), c(b + 1)}.
 * A record is four int32.  threshold is per call, in [1, 16384] in units of 2^-14 (2458 is about 0.15). */
typedef struct pv_f0_config {
    int32_t struct_size;     /* sizeof(pv_f0_config) as the caller compiled it (PV_F0_CONFIG_INIT sets it)                        */
    int32_t window;          /* W, the samples summed per lag                                                                    */
    int32_t hop;             /* samples between frames                                                                           */
    int32_t min_lag;         /* the shortest period looked for                                                                   */
    int32_t max_lag;         /* the lags computed; the longest period looked for is max_lag - 1                                  */
    int32_t max_channels;    /* channels per call (0 => 1), at most 65535                                                        */
    int32_t max_frames;      /* host-pointer calls: staging size in frames (0 => 256); longer calls go in pieces                 */
    int32_t device_id;       /* HIP device ordinal                                                                               */
    int32_t flags;           /* must be 0                                                                                        */
} pv_f0_config;
#define PV_F0_CONFIG_INIT { (int32_t)sizeof(pv_f0_config), 0, 0, 0, 0, 0, 0, 0, 0 }

typedef struct pv_f0 pv_f0;

/* Config errors are returned before any device is touched; failures are readable through pv_f0_last_error(NULL). */
PV_API int pv_f0_create(const pv_f0_config *cfg, pv_f0 **out);
PV_API int pv_f0_destroy(pv_f0 *h);
PV_API const char *pv_f0_last_error(const pv_f0 *h);
/* Use an externally owned hipStream_t; NULL => the handle's own stream. */
PV_API int pv_f0_set_stream(pv_f0 *h, void *hip_stream);
PV_API int pv_f0_synchronize(pv_f0 *h);
/* nframes frames of channels 0 .. nch-1: channel c reads in[c*in_stride .. + (nframes - 1) hop + W + max_lag) and writes nframes records to
 * records[4 (c*rec_stride + m) ..): rec_stride counts records.  Rejected with PV_ERR_ARGUMENT before any device work: a null buffer, a negative count,
 * a threshold outside [1, 16384] and, with nch > 1, strides below what a channel reads and writes.  nch > max_channels: PV_ERR_CAPACITY.  Host
 * pointers, synchronous, staged in pieces of max_frames. */
PV_API int pv_f0_track(pv_f0 *h, const float *in, int32_t nch, int64_t nframes, int64_t in_stride, int32_t threshold, int32_t *records, int64_t rec_stride);
/* The same on DEVICE in / records pointers (records 16-byte aligned: a record is one store), asynchronous on the handle's stream. */
PV_API int pv_f0_track_device(pv_f0 *h, const float *d_in, int32_t nch, int64_t nframes, int64_t in_stride, int32_t threshold, int32_t *d_records,
                              int64_t rec_stride);
/* Pure host code.  The period of one record in samples, fp64: tau + 0.5 (c- - c+) / (c- - 2 c0 + c+) when that denominator is positive, else tau;
 * 0 for an unvoiced or empty record. */
PV_API double pv_f0_period(const int32_t rec[4]);

/* Pitch correction onto a scale: from one channel's records to the hop row of pv_glide_process.  Frame by frame, with S the input consumed so far:
 * the record j = clamp((S + shift - f0_center + f0_hop div 2) div f0_hop, 0, nrec - 1) (floor division) has the period p; when p > 0,
 * n = 69 + 12 log2(sample_rate / p / a4), n* is the allowed note nearest n (ties to the lower) and t = strength (n* - n) / 12, else t = 0.  Then
 * r += retune (t - r), x = e + synthesis_hop / 2^r, hop = clamp(floor(x + 0.5), min_hop, max_hop), e = x - hop (the error diffusion of the bindings'
 * tempo_hops); the plan ends before the frame with S + hop > input_len. */
typedef struct pv_tune_params {
    int32_t struct_size;     /* sizeof(pv_tune_params) as the caller compiled it (PV_TUNE_PARAMS_INIT sets it)                    */
    int32_t f0_hop;          /* the tracker's hop                                                                                */
    int32_t f0_center;       /* where in its span a record is taken to sit, normally (W + max_lag) / 2                           */
    int32_t scale_mask;      /* 12 bits, bit k = pitch class k is allowed, C = 0; 0xFFF is chromatic; 0 is an error              */
    int32_t synthesis_hop;   /* the glide's                                                                                      */
    int32_t min_hop;         /* the glide's                                                                                      */
    int32_t max_hop;         /* the glide's                                                                                      */
    int32_t reserved;        /* must be 0                                                                                        */
    double sample_rate;      /* in Hz                                                                                            */
    double a4;               /* the reference pitch of note 69 in Hz; 0 => 440                                                   */
    double strength;         /* 0 .. 1: how much of the way to the note                                                          */
    double retune;           /* (0, 1]: the one-pole speed per frame, 1 jumps                                                    */
    int64_t input_len;       /* samples per channel of the input                                                                 */
    int64_t shift;           /* the caller's compensation for the glide's content lag, in input samples; may be 0                */
} pv_tune_params;
#define PV_TUNE_PARAMS_INIT { (int32_t)sizeof(pv_tune_params), 0, 0, 0xFFF, 0, 0, 0, 0, 0.0, 440.0, 1.0, 1.0, 0, 0 }
/* Returns the number of frames planned and writes at most `capacity` of them (the two-call sizing of pv_transient_plan): hops[m], and when curve is
 * not NULL the shift r of frame m in octaves.  records: nrec records of one channel, contiguous.  -PV_ERR_ARGUMENT for an argument out of range. */
PV_API int64_t pv_tune_plan(const pv_tune_params *p, const int32_t *records, int64_t nrec, int32_t *hops, double *curve, int64_t capacity);

/* ---- formant-preserving pitch correction: pitch-synchronous overlap-add (TD-PSOLA) on a grain table ------------------------------------ */
/* For a monophonic voice.  Two-period Hann grains are cut at the pitch period, re-spaced at period / ratio and overlap-added: a grain keeps the
 * vocal tract's response, so the spectral envelope stays where it was and only the spacing, the pitch, moves; duration is kept by construction.
 * The marks are spaced at the period, and aligned to the glottal epochs when the plan is made with epoch records (pv_epoch_plan below; DESIGN.md
 * "Pitch-synchronous correction" has the measured cost of unaligned marks), and one grain table serves every channel of a call, so a stereo pair keeps its image.
 * A grain is four int32 {t, tf, dq, L}: a Hann window of half length L samples centred at output position t + tf / 256 (tf in 0 .. 255) over the
 * input shifted by dq / 256 samples, i.e. output n of the grain reads the input at the real position n - dq / 256.  2 <= L <= max_period <= 4096,
 * |dq| <= 256 max_period, centres non-decreasing, positions relative to the buffer and below 2^30.  For output n and grain g:
 *   window   ua = |256 (n - t) - tf|; the weight is 0 when ua >= 256 L, else q = (4 ua) div L, rem = (4 ua) mod L, f = f32(rem) * (1.0f / f32(L)) and
 *            h = fmaf(f, Hn[q + 1] - Hn[q], Hn[q]) with the table Hn of pv_psola_window.
 *   sample   D = dq div 256, phi = dq mod 256 (floored).  phi == 0: the sample x[n - D] itself, so an unshifted grain is transparent.  Else
 *            theta = 256 - phi, b = n - D - 1 and 64 taps i = 0 .. 63 read x[b - 31 + i] with weight w_i = P[|256 (i - 31) - theta|], P the table of
 *            pv_vari_prototype used without interpolation: a = fmaf(w_i, x_i, a) and s = s + w_i for i ascending, xt = a / s.  x is 0 outside [0, nin).
 *   output   for the grains g ascending with h != 0: num = fmaf(h, xt, num), den = den + h; y[n] = num / den, or 0 where no grain covers n.
 * The order of every sum is a function of (g, i) alone: outputs [out_first, out_first + nout) are a pure function of (buffer, grains), and any
 * partition of the range into calls gives the same bits.  y[n] is non-finite exactly when a non-finite sample lies under a tap of a grain with
 * h != 0 (all 64 taps, or the one sample when phi == 0). */
typedef struct pv_psola_config {
    int32_t struct_size;     /* sizeof(pv_psola_config) as the caller compiled it (PV_PSOLA_CONFIG_INIT sets it)                  */
    int32_t max_period;      /* the largest half length L and the largest |dq| / 256 a call may pass, 2 .. 4096                  */
    int32_t max_channels;    /* channels per call (0 => 1), at most 65535                                                        */
    int32_t max_outputs;     /* host-pointer calls: staging size in outputs (0 => 65536), rounded up to whole tiles of 1024       */
    int32_t device_id;       /* HIP device ordinal                                                                               */
    int32_t flags;           /* must be 0                                                                                        */
} pv_psola_config;
#define PV_PSOLA_CONFIG_INIT { (int32_t)sizeof(pv_psola_config), 0, 0, 0, 0, 0 }

typedef struct pv_psola pv_psola;

/* Config errors are returned before any device is touched; failures are readable through pv_psola_last_error(NULL). */
PV_API int pv_psola_create(const pv_psola_config *cfg, pv_psola **out);
PV_API int pv_psola_destroy(pv_psola *h);
PV_API const char *pv_psola_last_error(const pv_psola *h);
/* Use an externally owned hipStream_t; NULL => the handle's own stream. */
PV_API int pv_psola_set_stream(pv_psola *h, void *hip_stream);
PV_API int pv_psola_synchronize(pv_psola *h);
/* Outputs [out_first, out_first + nout) of channels 0 .. nch-1: channel c reads in[c*in_stride .. + nin) and writes out[c*out_stride .. + nout),
 * out[0] being output out_first.  grains: ngrains records of four int32 on the HOST, one table for all channels.  Stateless.  Rejected with
 * PV_ERR_ARGUMENT before any device work and with the output untouched: a null buffer, a negative count, a position of 2^30 or more, with nch > 1
 * strides below nin / nout, and a grain out of range or out of order (the message names the grain).  nch > max_channels: PV_ERR_CAPACITY.  Host
 * pointers, synchronous, staged in pieces of max_outputs. */
PV_API int pv_psola_process(pv_psola *h, const float *in, int64_t nin, int64_t in_stride, int32_t nch, const int32_t *grains, int64_t ngrains, float *out,
                            int64_t out_first, int64_t nout, int64_t out_stride);
/* The same on DEVICE in / out pointers (grains stay a host table), asynchronous on the handle's stream. */
PV_API int pv_psola_process_device(pv_psola *h, const float *d_in, int64_t nin, int64_t in_stride, int32_t nch, const int32_t *grains, int64_t ngrains,
                                   float *d_out, int64_t out_first, int64_t nout, int64_t out_stride);
/* Pure host code, no handle and no device: the window table Hn, 1026 floats, Hn[q] = f32((1 + cos(pi q / 1024)) / 2) for q < 1024 and two zeros, with
 * the two-call sizing of pv_vari_prototype. */
PV_API int64_t pv_psola_window(float *table, int64_t capacity);

/* One pitch ratio per f0 record, pure host code: the target rule of pv_tune_plan (scale_mask, strength, a4, sample_rate; the hop fields, input_len and
 * shift are ignored) with the one-pole running per RECORD: r_j = r_(j-1) + retune (t_j - r_(j-1)), t_j = 0 for an unvoiced or empty record, and
 * ratios[j] = 2^r_j held within [1/2, 2].  Returns nrec and writes at most `capacity` ratios; -PV_ERR_ARGUMENT for an argument out of range. */
PV_API int64_t pv_psola_ratios(const pv_tune_params *p, const int32_t *records, int64_t nrec, double *ratios, int64_t capacity);

/* The grain table that moves every voiced stretch by its ratio.  rec(x) = clamp((floor(x) - f0_center + f0_hop div 2) div f0_hop, 0, nrec - 1);
 * P(x) is pv_f0_period of that record held within [min_period, max_period], unvoiced_period where it is 0 (and without records); rho(x) its ratio,
 * 1 where it is unvoiced or ratios is NULL.  Analysis marks A_0 = 0, A_(i+1) = A_i + P(A_i); synthesis marks T_0 = 0,
 * T_(k+1) = T_k + min(P(T_k) / rho(T_k), cap), cap = max(2 max_period - 4, 1), while T_k < input_len, all in fp64.  Grain k takes the analysis mark
 * A_i nearest T_k (ties to the lower; a monotone walk).  Where both T_k and A_i fall on unvoiced records, A_i < input_len and
 * 1 <= A_i - T_(k-1) <= cap, T_k becomes A_i: unvoiced material passes unshifted.  Then c = floor(256 T_k + 1/2), t = c div 256, tf = c mod 256,
 * dq = floor(256 (T_k - A_i) + 1/2) and L = clamp(max(floor(P(A_i) + 1/2), floor(g / 2) + 2), 2, max_period), g the larger of the distances to the
 * marks before and after T_k (after the last one: to where the next would be), so that neighbouring grains always overlap.  Centres are strictly
 * ascending and |dq| <= 128 max_period + 256. */
typedef struct pv_psola_params {
    int32_t struct_size;     /* sizeof(pv_psola_params) as the caller compiled it (PV_PSOLA_PARAMS_INIT sets it)                  */
    int32_t f0_hop;          /* the tracker's hop                                                                                */
    int32_t f0_center;       /* where in its span a record is taken to sit, normally (W + max_lag) / 2                           */
    int32_t min_period;      /* >= 2: shorter periods are held here                                                              */
    int32_t max_period;      /* <= 4096: longer periods are held here; no half length exceeds it (the handle's max_period)       */
    int32_t reserved;        /* must be 0                                                                                        */
    double unvoiced_period;  /* the mark spacing where there is no pitch, within [min_period, max_period]                        */
    int64_t input_len;       /* samples per channel of the input, below 2^30                                                     */
} pv_psola_params;
#define PV_PSOLA_PARAMS_INIT { (int32_t)sizeof(pv_psola_params), 0, 0, 0, 0, 0, 0.0, 0 }
/* Returns the number of grains planned and writes at most `capacity` of them (four int32 each; the two-call sizing of pv_transient_plan).  records:
 * nrec records of one channel; ratios: nrec values within [1/2, 2] or NULL.  -PV_ERR_ARGUMENT for an argument out of range. */
PV_API int64_t pv_psola_plan(const pv_psola_params *p, const int32_t *records, int64_t nrec, const double *ratios, int32_t *grains, int64_t capacity);

/* ---- epoch marks for the overlap-add path: where the pitch pulses sit (a separate handle) and the planner that puts the analysis marks there ---- */
/* A comb of short-time energy steps at the pitch period, on block-scaled integers: every value of a record is an exact integer function of the frame's
 * samples and of its period, whatever the tiling.  Per channel, frame m reads the `window` samples x[m hop, m hop + window) and nothing else: no
 * padding, no carried state; and one int32 p = periods256[m], the period in 1/256 sample (pv_epoch_periods makes the row from f0 records; one row
 * serves all channels, as the grain table does).  8 <= max_period <= 2048, 2 max_period <= window <= 8192, 1 <= hop <= 4096.
 *   scale    A = max |x_i| in f32; a non-finite sample, A == 0 or a p outside [256 * 8, 256 max_period] give the record {0, 0, 0, 0} (such a p is data,
 *            not an error).  Else A = f 2^e with f in [0.5, 1) and q_i = rint(x_i 2^(10 - e)), exactly scaled, ties to even: |q_i| <= 1024.
 *   sizes    w = max(2, p >> 10), a quarter period; Pc = (p + 255) >> 8; S(a, b) = sum_{a <= i < b} q_i^2.
 *   rise     D[n] = S(n, n + w) - S(n - w, n), the step in short-time energy at n, and the mass M[n] = S(n - w, n + w), for w <= n <= window - w.
 *   comb     K = the number of k >= 0 with w + Pc - 1 + ((k p) >> 8) <= window - w (at least 1);
 *            C(phi) = sum_{k < K} D[w + phi + ((k p) >> 8)] for phi = 0 .. Pc - 1, in int64; phi* is the first argmax.
 *   record   {w + phi*, K, w, s}: the position in the frame of the first pulse found, the teeth summed, the quarter period, and the strength
 *            s = (max(C(phi*), 0) 2^14) div Mtot, Mtot = sum_{k < K} M[w + phi* + ((k p) >> 8)], s = 0 when Mtot == 0; 0 <= s <= 16384.
 * A record is four int32.  The position trails the pulse of a voice by a few samples, the same few at every phase (DESIGN.md "Epoch marks"). */
typedef struct pv_epoch_config {
    int32_t struct_size;     /* sizeof(pv_epoch_config) as the caller compiled it (PV_EPOCH_CONFIG_INIT sets it)                  */
    int32_t window;          /* samples per frame                                                                                */
    int32_t hop;             /* samples between frames: the f0 tracker's hop when the records go to pv_epoch_plan                */
    int32_t max_period;      /* the longest period looked for, in samples                                                        */
    int32_t max_channels;    /* channels per call (0 => 1), at most 65535                                                        */
    int32_t max_frames;      /* host-pointer calls: staging size in frames (0 => 256); longer calls go in pieces                 */
    int32_t device_id;       /* HIP device ordinal                                                                               */
    int32_t flags;           /* must be 0                                                                                        */
} pv_epoch_config;
#define PV_EPOCH_CONFIG_INIT { (int32_t)sizeof(pv_epoch_config), 0, 0, 0, 0, 0, 0, 0 }

typedef struct pv_epoch pv_epoch;

/* Config errors are returned before any device is touched; failures are readable through pv_epoch_last_error(NULL). */
PV_API int pv_epoch_create(const pv_epoch_config *cfg, pv_epoch **out);
PV_API int pv_epoch_destroy(pv_epoch *h);
PV_API const char *pv_epoch_last_error(const pv_epoch *h);
/* Use an externally owned hipStream_t; NULL => the handle's own stream. */
PV_API int pv_epoch_set_stream(pv_epoch *h, void *hip_stream);
PV_API int pv_epoch_synchronize(pv_epoch *h);
/* nframes frames of channels 0 .. nch-1: channel c reads in[c*in_stride .. + (nframes - 1) hop + window) and periods256[0 .. nframes) and writes nframes
 * records to records[4 (c*rec_stride + m) ..): rec_stride counts records.  Rejected with PV_ERR_ARGUMENT before any device work and with the records
 * untouched: a null buffer, a negative count and, with nch > 1, strides below what a channel reads and writes.  nch > max_channels: PV_ERR_CAPACITY.
 * Host pointers, synchronous, staged in pieces of max_frames. */
PV_API int pv_epoch_track(pv_epoch *h, const float *in, int32_t nch, int64_t nframes, int64_t in_stride, const int32_t *periods256, int32_t *records,
                          int64_t rec_stride);
/* The same on DEVICE in / periods / records pointers (records 16-byte aligned: a record is one store), asynchronous on the handle's stream. */
PV_API int pv_epoch_track_device(pv_epoch *h, const float *d_in, int32_t nch, int64_t nframes, int64_t in_stride, const int32_t *d_periods256,
                                 int32_t *d_records, int64_t rec_stride);
/* Pure host code.  The period row of pv_epoch_track from f0 records: periods256[j] = floor(256 pv_f0_period(record j) + 1/2), 0 where it is unvoiced or
 * empty.  Returns nrec and writes at most `capacity` values (the two-call sizing of pv_transient_plan); -PV_ERR_ARGUMENT for an argument out of range. */
PV_API int64_t pv_epoch_periods(const int32_t *records, int64_t nrec, int32_t *periods256, int64_t capacity);

/* pv_psola_plan with its analysis marks on the pulses.  epochs: nrec epoch records, record j belonging to f0 record j with its position relative to
 * j f0_hop (an epoch handle run at the tracker's hop on the same buffer), or NULL.  Everything is pv_psola_plan's but the analysis marks:
 * A_0 = snap(0, none), A_(i+1) = snap(A_i + P(A_i), A_i).  snap(c, prev), with j = rec(c): c itself when epochs is NULL, f0 record j is unvoiced,
 * K_j <= 0 or s_j < min_strength.  Else P = P(c), E = j f0_hop + pos_j and s = E + floor((c - E) / P + 1/2) P, the lattice point nearest c; when prev is
 * given and s - prev < P / 2, s += P; when prev is given, voiced(prev) and |s - c| <= P / 4, s = c + lock (s - c): a first-order lock, so that the
 * half-sample quantisation of the records does not become mark jitter, while a larger disagreement and the first voiced mark after an unvoiced one
 * snap at once.  With epochs == NULL the grains are pv_psola_plan's bit for bit.  Centres are strictly ascending and |dq| <= 256 max_period. */
typedef struct pv_epoch_params {
    int32_t struct_size;     /* sizeof(pv_epoch_params) as the caller compiled it (PV_EPOCH_PARAMS_INIT sets it)                  */
    int32_t min_strength;    /* 0 .. 16384: records with a smaller s leave their marks where pv_psola_plan puts them             */
    double lock;             /* (0, 1]: how much of a small correction one mark takes; 1 snaps every mark                        */
} pv_epoch_params;
#define PV_EPOCH_PARAMS_INIT { (int32_t)sizeof(pv_epoch_params), 0, 0.125 }
/* Returns the number of grains planned and writes at most `capacity` of them, as pv_psola_plan.  -PV_ERR_ARGUMENT for an argument out of range. */
PV_API int64_t pv_epoch_plan(const pv_psola_params *p, const pv_epoch_params *e, const int32_t *records, int64_t nrec, const double *ratios,
                             const int32_t *epochs, int32_t *grains, int64_t capacity);

/* ---- time-scale modification on the overlap-add path: the output runs at another speed than the input, pitch and formants stay (a separate handle) ---- */
/* TD-PSOLA's duration half.  pv_psola_process writes every grain near where it reads (|dq| <= 256 max_period): the output is as long as the input.
 * Here a grain reads the input anywhere.  A far grain is four int32 {t, w, D, L} with w = tf + 256 phi, tf and phi in 0 .. 255: a Hann window of half
 * length L centred at output position t + tf / 256; output n of the grain reads the input at the real position n - D - phi / 256.  D is any whole number
 * with |D| < 2^30: it stands where pv_psola's dq div 256 stands, and phi where its dq mod 256.  2 <= L <= max_period, 0 <= t < 2^30, centres
 * non-decreasing.  The window, sample and output rules are pv_psola_process's word for word (the same Hn and P; phi == 0 reads x[n - D] itself, else
 * theta = 256 - phi, b = n - D - 1 and 64 taps; num and den in grain order; x is 0 outside [0, nin)), so a table whose grains all have
 * |256 D + phi| <= 256 max_period is pv_psola_process's table in another notation and gives its bits.  The order of every sum is a function of (g, i)
 * alone: any partition of the output range into calls gives the same bits.
 * What a call may read: its outputs go in tiles of 1024 from out_first on, and the input samples that the grains reaching one tile [j0, j1) read inside it,
 * from min (max(j0, t - L) - D - 33) to max (min(j1, t + L) - D + 32), must not be more than
 * span(max_period, max_rate) = max_rate (1024 + 2 max_period) + 4 max_period + 64.  A table of pv_tsm_plan whose rates lie within
 * [1 / max_rate, max_rate] keeps to it (DESIGN.md "Time-scale modification"); a call with a tile beyond it is refused.  The span, the prototype and the
 * window table share the 160 KiB of LDS of a compute unit: pv_tsm_create returns PV_ERR_UNSUPPORTED for a pair beyond that (max_period 4096 goes with
 * max_rate 1 only, 2048 and less with any).
 * Limits: for a monophonic voice; one plan serves all channels; unvoiced grains repeated at slow rates can buzz (their time direction is not alternated
 * here: pv_mirror_* below alternates it). */
typedef struct pv_tsm_config {
    int32_t struct_size;     /* sizeof(pv_tsm_config) as the caller compiled it (PV_TSM_CONFIG_INIT sets it)                      */
    int32_t max_period;      /* the largest half length L a call may pass, 2 .. 4096                                             */
    int32_t max_rate;        /* 1 .. 4: sizes the span; plans whose rates lie within [1 / max_rate, max_rate] fit                */
    int32_t max_channels;    /* channels per call (0 => 1), at most 65535                                                        */
    int32_t max_outputs;     /* host-pointer calls: staging size in outputs (0 => 65536), rounded up to whole tiles of 1024       */
    int32_t device_id;       /* HIP device ordinal                                                                               */
    int32_t flags;           /* must be 0                                                                                        */
} pv_tsm_config;
#define PV_TSM_CONFIG_INIT { (int32_t)sizeof(pv_tsm_config), 0, 0, 0, 0, 0, 0 }

typedef struct pv_tsm pv_tsm;

/* Config errors are returned before any device is touched; failures are readable through pv_tsm_last_error(NULL). */
PV_API int pv_tsm_create(const pv_tsm_config *cfg, pv_tsm **out);
PV_API int pv_tsm_destroy(pv_tsm *h);
PV_API const char *pv_tsm_last_error(const pv_tsm *h);
/* Use an externally owned hipStream_t; NULL => the handle's own stream. */
PV_API int pv_tsm_set_stream(pv_tsm *h, void *hip_stream);
PV_API int pv_tsm_synchronize(pv_tsm *h);
/* Outputs [out_first, out_first + nout) of channels 0 .. nch-1: channel c reads in[c*in_stride .. + nin) and writes out[c*out_stride .. + nout),
 * out[0] being output out_first; nout is the caller's (pv_tsm_plan's output_len for a whole signal).  grains: ngrains far grains on the HOST, one table
 * for all channels.  Stateless.  Rejected with PV_ERR_ARGUMENT before any device work and with the output untouched: a null buffer, a negative count, a
 * position of 2^30 or more, with nch > 1 strides below nin / nout, a grain out of range or out of order, and a tile that reads more than the span (the
 * message names the grain, for a tile its first).  nch > max_channels: PV_ERR_CAPACITY.  Host pointers, synchronous, staged in pieces of max_outputs
 * or less: a piece stages the input range its tiles read, and is one tile where more would not fit the staging buffer. */
PV_API int pv_tsm_process(pv_tsm *h, const float *in, int64_t nin, int64_t in_stride, int32_t nch, const int32_t *grains, int64_t ngrains, float *out,
                          int64_t out_first, int64_t nout, int64_t out_stride);
/* The same on DEVICE in / out pointers (grains stay a host table), asynchronous on the handle's stream. */
PV_API int pv_tsm_process_device(pv_tsm *h, const float *d_in, int64_t nin, int64_t in_stride, int32_t nch, const int32_t *grains, int64_t ngrains,
                                 float *d_out, int64_t out_first, int64_t nout, int64_t out_stride);
/* Pure host code: pv_epoch_plan with a read position V beside the synthesis position T, V_0 = T_0 = 0.  rates: nrec values, rates[j] the input samples
 * consumed per output sample while V lies on record j (2 plays twice as fast, 1/2 at half speed), finite and positive, held within [1/4, 4], voiced or
 * not; NULL: 1.  Everything is pv_epoch_plan's (rec, P, rho, snap, the marks A_i, the monotone walk, c / t / tf / L of a grain, cap) with two
 * differences: the loop runs while V < input_len, and the walk takes the mark nearest V, with step, voiced, rho and rate evaluated at V.  After a grain
 * is held, s = min(P(V) / rho(V), cap), T += s, V += rate(V) s.  A grain has dq = floor(256 (T - A) + 1/2) in int64, D = dq div 256, phi = dq mod 256.
 * Where a grain is held, neither V nor A is voiced and A < input_len: Tn = A + rint((T + (A - V)) - A), and if A >= Vprev + 1, Tn >= Tprev + 1 and
 * Tn - Tprev <= cap then T = Tn, V = A: unvoiced material passes as whole-sample copies at any rate (there the rate is realised as a pattern of mark
 * reuse, exactly where it or its inverse is whole).  *output_len (may be NULL) = floor(T + (input_len - V) / rate(V) + 1/2) for the last grain's T
 * and V, 0 without grains.  With rates == NULL the grains are pv_epoch_plan's in the far notation, bit for bit, and output_len == input_len.
 * Returns the number of grains and writes at most `capacity` of them, as pv_psola_plan; -PV_ERR_ARGUMENT for an argument out of range, and when a
 * centre would reach 2^30 (grains before it may have been written). */
PV_API int64_t pv_tsm_plan(const pv_psola_params *p, const pv_epoch_params *e, const int32_t *records, int64_t nrec, const double *ratios,
                           const double *rates, const int32_t *epochs, int32_t *grains, int64_t capacity, int64_t *output_len);

/* ---- mirrored grains on the overlap-add path: a grain may read the input backwards, so that a repeated noise grain does not buzz (a separate handle) ---- */
/* At a rate below 1 pv_tsm_plan uses every analysis mark of an unvoiced stretch two or three times; the same noise grain repeating at the mark spacing
 * is heard as a tone at sample_rate / unvoiced_period.  TD-PSOLA's remedy is to alternate the time direction of the repeats.  A grain here is
 * pv_tsm_process's {t, w, D, L} with one more bit: w = tf + 256 phi + 65536 m, m in {0, 1}, 0 <= w < 131072.  With m = 0 it is pv_tsm_process's far grain
 * word for word (|D| < 2^30), and a table without mirrored grains gives pv_tsm_process's bits.  With m = 1 the grain is mirrored: output n reads the
 * input at the real position D - n - phi / 256; D > -2^30, any larger int32 is allowed (D is a sum of two positions below 2^30).  The window and output
 * rules do not change; the sample rule is the forward one with n - D replaced by D - n and nothing else (phi == 0 reads x[D - n] itself, else
 * theta = 256 - phi, b = D - n - 1 and the 64 taps x[b - 31 + i] with weights P[|256 (i - 31) - theta|], i ascending).  The order of every sum stays a
 * function of (g, i) alone: any partition of the output range into calls gives the same bits.
 * What a call may read: pv_tsm_process's rule, with the source range of a mirrored grain that reaches the tile [j0, j1) running from
 * D - min(j1, t + L) - 33 to D - max(j0, t - L) + 32; span(max_period, max_rate) and the 160 KiB rule of pv_tsm_create are unchanged, and a table of
 * pv_mirror_plan whose rates lie within [1 / max_rate, max_rate] keeps to the span (DESIGN.md "Mirrored grains").
 * Limits: pv_tsm's; with three or more uses of one mark the first and the third are both forward, so a component at twice the mark spacing stays. */
typedef struct pv_mirror_config {
    int32_t struct_size;     /* sizeof(pv_mirror_config) as the caller compiled it (PV_MIRROR_CONFIG_INIT sets it)                */
    int32_t max_period;      /* the largest half length L a call may pass, 2 .. 4096                                             */
    int32_t max_rate;        /* 1 .. 4: sizes the span, as pv_tsm_config                                                         */
    int32_t max_channels;    /* channels per call (0 => 1), at most 65535                                                        */
    int32_t max_outputs;     /* host-pointer calls: staging size in outputs (0 => 65536), rounded up to whole tiles of 1024       */
    int32_t device_id;       /* HIP device ordinal                                                                               */
    int32_t flags;           /* must be 0                                                                                        */
} pv_mirror_config;
#define PV_MIRROR_CONFIG_INIT { (int32_t)sizeof(pv_mirror_config), 0, 0, 0, 0, 0, 0 }

typedef struct pv_mirror pv_mirror;

/* Config errors are returned before any device is touched, PV_ERR_UNSUPPORTED where pv_tsm_create returns it; failures are readable through
 * pv_mirror_last_error(NULL). */
PV_API int pv_mirror_create(const pv_mirror_config *cfg, pv_mirror **out);
PV_API int pv_mirror_destroy(pv_mirror *h);
PV_API const char *pv_mirror_last_error(const pv_mirror *h);
/* Use an externally owned hipStream_t; NULL => the handle's own stream. */
PV_API int pv_mirror_set_stream(pv_mirror *h, void *hip_stream);
PV_API int pv_mirror_synchronize(pv_mirror *h);
/* Outputs [out_first, out_first + nout) of channels 0 .. nch-1, with pv_tsm_process's arguments and layout; grains is a HOST table, one for all
 * channels.  Stateless.  Rejected with PV_ERR_ARGUMENT before any device work and with the output untouched: everything pv_tsm_process rejects, with
 * the grain rules above (w of 131072 or more, a mirrored grain with D <= -2^30, a forward grain with |D| >= 2^30), and a tile that reads more than the
 * span (the message names the grain, for a tile its first).  nch > max_channels: PV_ERR_CAPACITY.  Host pointers, synchronous, staged in pieces of
 * whole tiles as pv_tsm_process: a piece stages the hull of its tiles' source ranges cut to the input. */
PV_API int pv_mirror_process(pv_mirror *h, const float *in, int64_t nin, int64_t in_stride, int32_t nch, const int32_t *grains, int64_t ngrains, float *out,
                             int64_t out_first, int64_t nout, int64_t out_stride);
/* The same on DEVICE in / out pointers (grains stay a host table), asynchronous on the handle's stream. */
PV_API int pv_mirror_process_device(pv_mirror *h, const float *d_in, int64_t nin, int64_t in_stride, int32_t nch, const int32_t *grains, int64_t ngrains,
                                    float *d_out, int64_t out_first, int64_t nout, int64_t out_stride);
/* Pure host code: pv_tsm_plan with the direction of every grain.  mirror == 0: pv_tsm_plan's grains and output_len bit for bit.  mirror == 1 (any other
 * value is refused): the walk, the marks, T, V, c, L and output_len do not change.  A grain held at (T, A) is a REUSE when a grain was held before it,
 * that grain's analysis mark is this very A (the same double: the walk did not advance) and the record at A is unvoiced or there are no records.  A
 * reuse takes the opposite direction of the grain before it; every other grain is forward, so a voiced grain is never mirrored.  A mirrored grain reads
 * about its own mark (input A - (tau - T) lands at output tau): sq = floor(256 (T + A) + 1/2) in int64, D = (sq + 255) >> 8, phi = 256 D - sq,
 * w = tf + 256 phi + 65536.  Returns and refuses as pv_tsm_plan (and refuses a plan whose mirrored D would pass int32). */
PV_API int64_t pv_mirror_plan(const pv_psola_params *p, const pv_epoch_params *e, const int32_t *records, int64_t nrec, const double *ratios,
                              const double *rates, const int32_t *epochs, int32_t mirror, int32_t *grains, int64_t capacity, int64_t *output_len);

/* ---- formant shifting on the overlap-add path: a grain may read the input at a step of its own, which moves the spectral envelope (a separate handle) ---- */
/* The overlap-add path moves pitch and tempo and keeps the formants where they were; this moves them on purpose (the "throat" control).  A grain that reads
 * its input at a step other than one sample per output sample is time-compressed or time-expanded, which scales its spectrum, and so the envelope, by that
 * step; the grain spacing still sets the pitch.  A grain here is pv_tsm_process's {t, w, D, L} with a step: w = tf + 256 phi + 131072 z, 0 <= w < 2^27,
 * bit 16 (pv_mirror's direction bit) 0.  z is the step s in 1/256: z = 0 means s = 256, else 128 <= z <= 512 and s = z; z = 256 is treated exactly as z = 0.
 * With s = 256 the grain is pv_tsm_process's far grain word for word, and a table without warped grains gives pv_tsm_process's bits.  With s != 256 output
 * n of the grain reads the input at the real position (t + tf / 256 - D - phi / 256) + (s / 256) (n - t - tf / 256), in exact integers: u = 256 (n - t) - tf,
 * v = 256 (tf - phi) + s u, m = (t - D) + floor(v / 65536), r = v mod 65536; den = max(256, s), W = 32 for s <= 256 and 64 otherwise; tap i = 0 .. 2 W - 1
 * reads x[m - W + 1 + i] with d = |(i - W + 1) 65536 - r|, q = d div den, rem = d mod den, weight 0 when q >= 8192, else
 * fmaf(f32(rem) * (1.0f / f32(den)), P[q + 1] - P[q], P[q]) (pv_vari's weight rule: above s = 256 the cutoff falls by 256 / s, so a compressed grain does
 * not alias); a = fmaf(w_i, x_i, a) and sum += w_i for i ascending, xt = a / sum; a tap whose weight is exactly 0 touches neither sum whatever its sample
 * holds.  Window, output rule and summation order are pv_tsm_process's: any partition of the output range into calls gives the same bits.
 * What a call may read: per tile of 1024 outputs the hull of its grains' source ranges (psola/pv_formant.h gives the range of a warped grain) may not exceed
 * span(max_period, max_rate) = max_rate (1024 + 2 max_period) + 6 max_period + 192 samples; a table of pv_formant_plan whose rates lie within
 * [1 / max_rate, max_rate] and whose warps lie within [1/2, 2] keeps to it.  The span, the prototype and the window table share the 160 KiB of LDS of a
 * compute unit, so fewer pairs fit than pv_tsm's: max_period up to 3753 at max_rate 1, 2900 at 2, 2331 at 3, 1925 at 4; pv_formant_create returns
 * PV_ERR_UNSUPPORTED beyond.
 * Limits: pv_tsm's; no mirrored warped grains; pv_harmony_* and pv_takes_* keep unwarped grains; a warp above about twice the pitch ratio leaves grains
 * longer than two of their periods (the planner's gap floor), which blurs the moved envelope. */
typedef struct pv_formant_config {
    int32_t struct_size;     /* sizeof(pv_formant_config) as the caller compiled it (PV_FORMANT_CONFIG_INIT sets it)              */
    int32_t max_period;      /* the largest half length L a call may pass, 2 .. 4096 (with max_rate: the LDS rule above)          */
    int32_t max_rate;        /* 1 .. 4: sizes the span, as pv_tsm_config                                                         */
    int32_t max_channels;    /* channels per call (0 => 1), at most 65535                                                        */
    int32_t max_outputs;     /* host-pointer calls: staging size in outputs (0 => 65536), rounded up to whole tiles of 1024       */
    int32_t device_id;       /* HIP device ordinal                                                                               */
    int32_t flags;           /* must be 0                                                                                        */
} pv_formant_config;
#define PV_FORMANT_CONFIG_INIT { (int32_t)sizeof(pv_formant_config), 0, 0, 0, 0, 0, 0 }

typedef struct pv_formant pv_formant;

/* Config errors are returned before any device is touched, PV_ERR_UNSUPPORTED for a pair beyond the LDS rule; failures are readable through
 * pv_formant_last_error(NULL). */
PV_API int pv_formant_create(const pv_formant_config *cfg, pv_formant **out);
PV_API int pv_formant_destroy(pv_formant *h);
PV_API const char *pv_formant_last_error(const pv_formant *h);
/* Use an externally owned hipStream_t; NULL => the handle's own stream. */
PV_API int pv_formant_set_stream(pv_formant *h, void *hip_stream);
PV_API int pv_formant_synchronize(pv_formant *h);
/* Outputs [out_first, out_first + nout) of channels 0 .. nch-1, with pv_tsm_process's arguments and layout; grains is a HOST table, one for all
 * channels.  Stateless.  Rejected with PV_ERR_ARGUMENT before any device work and with the output untouched: everything pv_tsm_process rejects, with
 * the grain rules above (w of 2^27 or more, a step of 1 .. 127 or above 512, a set bit 16), and a tile that reads more than the span (the message names the
 * grain, for a tile its first).  nch > max_channels: PV_ERR_CAPACITY.  Host pointers, synchronous, staged in pieces of whole tiles as pv_tsm_process. */
PV_API int pv_formant_process(pv_formant *h, const float *in, int64_t nin, int64_t in_stride, int32_t nch, const int32_t *grains, int64_t ngrains, float *out,
                              int64_t out_first, int64_t nout, int64_t out_stride);
/* The same on DEVICE in / out pointers (grains stay a host table), asynchronous on the handle's stream. */
PV_API int pv_formant_process_device(pv_formant *h, const float *d_in, int64_t nin, int64_t in_stride, int32_t nch, const int32_t *grains, int64_t ngrains,
                                     float *d_out, int64_t out_first, int64_t nout, int64_t out_stride);
/* Pure host code: pv_tsm_plan with one more row, warps[j], one step per f0 record, each within [1/2, 2] (else refused, as ratios are); above 1 the formants
 * move up.  warps == NULL: pv_tsm_plan's grains and output_len bit for bit.  Else the grain held for the analysis mark A takes alpha = warps[record of A],
 * voiced or not (consonants move with the vowels): s = floor(256 alpha + 1/2), z = 0 when s == 256 and s otherwise, and its half length starts from
 * floor(period(A) / (s / 256.0) + 1/2) in place of floor(period(A) + 1/2); pv_tsm_plan's floors then apply unchanged (at least floor(gap / 2) + 2, at
 * least 2, at most max_period).  Marks, read position, D, phi and output_len do not depend on warps.  Limit: where alpha is above about twice the ratio the
 * gap floor lengthens the grain beyond two of its periods; alpha is not clamped.  Returns and refuses as pv_tsm_plan. */
PV_API int64_t pv_formant_plan(const pv_psola_params *p, const pv_epoch_params *e, const int32_t *records, int64_t nrec, const double *ratios,
                               const double *rates, const double *warps, const int32_t *epochs, int32_t *grains, int64_t capacity, int64_t *output_len);

/* ---- harmony voices on the overlap-add path: several differently shifted copies of the voice summed into one output (a separate handle) ---- */
/* A harmonizer: a third and a fifth above the lead, in key, on the same time base.  A call has nvoices voices, 1 <= nvoices <= 8.  Voice v is a far-grain
 * table of pv_tsm_process, in its notation and under its rules word for word, and y_v[n] is exactly what pv_tsm_process gives for that table alone: one
 * num / den per voice (a merged table would normalise over all the grains that cover an output and average the voices instead of adding them).
 * gains[v nch + c] is a finite float per (voice, channel).  For channel c and output n: acc = 0.0f, and for v ascending, voice v is skipped when
 * gains[v nch + c] == 0 or no grain of voice v covers n with a non-zero weight (a skipped voice touches nothing: a NaN under the taps of a muted voice
 * stays out); else acc = acc + f32(gains[v nch + c] * y_v[n]), the product rounded to f32 on its own, then a plain add.  out[c][n] = acc, 0 where no voice
 * contributes.  So float32 arithmetic on the per-voice outputs of pv_tsm_process reproduces the mix bit for bit.  The order of every sum is a function of
 * (v, g, i) alone: any partition of the output range into calls gives the same bits.
 * grains is the concatenation of the voices' tables and voice_first[0 .. nvoices] gives the offsets in grains (records of four int32):
 * voice_first[0] == 0, non-decreasing, voice_first[nvoices] the number of grains; an empty voice is legal.  Centres are non-decreasing within a voice and
 * may restart at a voice boundary.
 * What a call may read: a tile's input is staged once for all voices, so the HULL over the voices of pv_tsm_process's per-voice source range of the tile
 * (voices with no grain on the tile left out) must not be more than span(max_period, max_rate) of pv_tsm_config; a call with a tile beyond it is
 * refused, even when every voice alone would fit.  Voices planned by pv_tsm_plan on one row of rates within [1 / max_rate, max_rate] keep to it
 * (DESIGN.md "Harmony voices").  pv_harmony_create returns PV_ERR_UNSUPPORTED where pv_tsm_create does.
 * Limits: for a monophonic voice; one row of rates for all voices; in unvoiced stretches every voice is the same unshifted copy, so consonants add up
 * nvoices-fold: the gains are the remedy. */
typedef struct pv_harmony_config {
    int32_t struct_size;     /* sizeof(pv_harmony_config) as the caller compiled it (PV_HARMONY_CONFIG_INIT sets it)              */
    int32_t max_period;      /* the largest half length L a call may pass, 2 .. 4096                                             */
    int32_t max_rate;        /* 1 .. 4: sizes the span, as pv_tsm_config                                                         */
    int32_t max_voices;      /* voices per call, 1 .. 8 (0 => 8)                                                                 */
    int32_t max_channels;    /* channels per call (0 => 1), at most 65535                                                        */
    int32_t max_outputs;     /* host-pointer calls: staging size in outputs (0 => 65536), rounded up to whole tiles of 1024       */
    int32_t device_id;       /* HIP device ordinal                                                                               */
    int32_t flags;           /* must be 0                                                                                        */
} pv_harmony_config;
#define PV_HARMONY_CONFIG_INIT { (int32_t)sizeof(pv_harmony_config), 0, 0, 0, 0, 0, 0, 0 }

typedef struct pv_harmony pv_harmony;

/* Config errors are returned before any device is touched; failures are readable through pv_harmony_last_error(NULL). */
PV_API int pv_harmony_create(const pv_harmony_config *cfg, pv_harmony **out);
PV_API int pv_harmony_destroy(pv_harmony *h);
PV_API const char *pv_harmony_last_error(const pv_harmony *h);
/* Use an externally owned hipStream_t; NULL => the handle's own stream. */
PV_API int pv_harmony_set_stream(pv_harmony *h, void *hip_stream);
PV_API int pv_harmony_synchronize(pv_harmony *h);
/* Outputs [out_first, out_first + nout) of channels 0 .. nch-1, as pv_tsm_process.  grains, voice_first and gains are HOST tables.  Stateless.  Rejected
 * with PV_ERR_ARGUMENT before any device work and with the output untouched: everything pv_tsm_process rejects, per voice (the message names voice and
 * grain, the grain counted within its voice), a malformed voice_first, nvoices < 1, a gain that is not finite, and a tile whose hull exceeds the span
 * (the message names the tile and the first grain of its lowest voice).  nvoices > max_voices or nch > max_channels: PV_ERR_CAPACITY.  Host pointers,
 * synchronous, staged in pieces of whole tiles as pv_tsm_process: a piece stages the hull of its tiles cut to the input. */
PV_API int pv_harmony_process(pv_harmony *h, const float *in, int64_t nin, int64_t in_stride, int32_t nch, const int32_t *grains, const int64_t *voice_first,
                              int32_t nvoices, const float *gains, float *out, int64_t out_first, int64_t nout, int64_t out_stride);
/* The same on DEVICE in / out pointers (grains, voice_first and gains stay host tables), asynchronous on the handle's stream. */
PV_API int pv_harmony_process_device(pv_harmony *h, const float *d_in, int64_t nin, int64_t in_stride, int32_t nch, const int32_t *grains,
                                     const int64_t *voice_first, int32_t nvoices, const float *gains, float *d_out, int64_t out_first, int64_t nout,
                                     int64_t out_stride);
/* Pure host code: one pitch ratio per (voice, f0 record), voice v a number of scale degrees away from the corrected lead.  r_j is pv_psola_ratios's
 * one-pole value, exactly, computed once for all voices.  For a voiced record take n, the allowed notes lo and hi on either side of it and the nearest
 * one ns as pv_psola_ratios does; voice v with k = degrees[v] moves from ns by |k| ALLOWED notes (those whose pitch class has its bit in scale_mask), up
 * for k > 0, down for k < 0, and i is that whole number of semitones; i = 0 for k = 0 and for unvoiced or empty records.
 * ratios[v capacity + j] = 2^(r_j + i / 12) held within [1/2, 2], for j < min(nrec, capacity).  So the correction glides with retune and the interval
 * jumps with the note; on the chromatic mask a degree is a semitone, on a seven-note mask degree 2 is a diatonic third; with k = 0 the row is
 * pv_psola_ratios's bit for bit.  The clamp limits a voice to an octave either way: a full octave on top of a correction in the same direction saturates.
 * Returns nrec (the two-call sizing of pv_psola_ratios, `capacity` being the length of a row); -PV_ERR_ARGUMENT for whatever pv_psola_ratios rejects,
 * nvoices outside [1, 8], a null degrees and |degrees[v]| > 24. */
PV_API int64_t pv_harmony_ratios(const pv_tune_params *p, const int32_t *records, int64_t nrec, const int32_t *degrees, int32_t nvoices, double *ratios,
                                 int64_t capacity);

/* ---- full-grain harmony voices on the overlap-add path: pv_harmony's voices, whose grains may be mirrored, warped or both (a separate handle) ---- */
/* What a harmonizer is bought for: a third below with the formants lowered (a different singer, not a chipmunk) beside the lead at warp 1, all at half
 * tempo without the unvoiced buzz, in one call.  pv_choir_* lifts the limits pv_formant_config states for its own handle: here a grain may be mirrored AND
 * warped, and every voice of a call carries the full grain word.  The structure is pv_harmony_process's (nvoices voices, grains the concatenation of the
 * voices' tables, voice_first, gains, one num / den per voice, the float32 gain fold in voice order, a skipped voice touches nothing); on tables of plain
 * far grains the output is pv_harmony_process's bit for bit.
 * A grain is {t, w, D, L} with w = tf + 256 phi + 65536 m + 131072 z, 0 <= w < 2^27: m is pv_mirror_process's direction bit and z pv_formant_process's step
 * s in 1/256 (z = 0 means s = 256, else 128 <= z <= 512; z = 256 is treated exactly as z = 0).  t, L and the ordering are pv_tsm_process's; D > -2^30
 * always and D < 2^30 only for a forward grain, as pv_mirror_process.  With m = 0, s = 256 the grain is pv_tsm_process's far grain word for word; with
 * m = 1, s = 256 pv_mirror_process's mirrored grain; with m = 0, s != 256 pv_formant_process's warped grain.  With m = 1 and s != 256 output n of the grain
 * reads the input at the real position (D - t - tf / 256 - phi / 256) - (s / 256) (n - t - tf / 256), in exact integers: u = 256 (n - t) - tf,
 * v = -256 (tf + phi) - s u, mm = (D - t) + floor(v / 65536), r = v mod 65536; from (mm, r) on the sample rule is pv_formant_process's, unchanged (tap i
 * reads x[mm - W + 1 + i] with d = |(i - W + 1) 65536 - r|).  At s = 256 that rule lands on the mirrored grain's positions and weights.
 * What a call may read: per tile of 1024 outputs the HULL over the voices of their grains' source ranges (psola/pv_choir.h gives the range of every kind
 * of grain) may not exceed span(max_period, max_rate) = max_rate (1024 + 2 max_period) + 6 max_period + 192 samples, pv_formant_config's span with its LDS
 * rule: max_period up to 3753 at max_rate 1, 2900 at 2, 2331 at 3, 1925 at 4; pv_choir_create returns PV_ERR_UNSUPPORTED beyond.  A call with a tile beyond
 * the span is refused, never clipped.  Voices planned by pv_choir_plan on one row of rates within [1 / max_rate, max_rate] with warps within [1/2, 2] keep
 * to it (DESIGN.md "Choir").
 * Limits: pv_harmony's (a monophonic voice; one row of rates for all voices; consonants add up nvoices-fold: the gains are the remedy) and the planner
 * limit of pv_formant_plan (a warp above about twice the pitch ratio leaves grains longer than two of their periods); pv_takes_* keeps unwarped grains. */
typedef struct pv_choir_config {
    int32_t struct_size;     /* sizeof(pv_choir_config) as the caller compiled it (PV_CHOIR_CONFIG_INIT sets it)                  */
    int32_t max_period;      /* the largest half length L a call may pass, 2 .. 4096 (with max_rate: the LDS rule above)          */
    int32_t max_rate;        /* 1 .. 4: sizes the span, as pv_formant_config                                                     */
    int32_t max_voices;      /* voices per call, 1 .. 8 (0 => 8)                                                                 */
    int32_t max_channels;    /* channels per call (0 => 1), at most 65535                                                        */
    int32_t max_outputs;     /* host-pointer calls: staging size in outputs (0 => 65536), rounded up to whole tiles of 1024       */
    int32_t device_id;       /* HIP device ordinal                                                                               */
    int32_t flags;           /* must be 0                                                                                        */
} pv_choir_config;
#define PV_CHOIR_CONFIG_INIT { (int32_t)sizeof(pv_choir_config), 0, 0, 0, 0, 0, 0, 0 }

typedef struct pv_choir pv_choir;

/* Config errors are returned before any device is touched, PV_ERR_UNSUPPORTED for a pair beyond the LDS rule; failures are readable through
 * pv_choir_last_error(NULL). */
PV_API int pv_choir_create(const pv_choir_config *cfg, pv_choir **out);
PV_API int pv_choir_destroy(pv_choir *h);
PV_API const char *pv_choir_last_error(const pv_choir *h);
/* Use an externally owned hipStream_t; NULL => the handle's own stream. */
PV_API int pv_choir_set_stream(pv_choir *h, void *hip_stream);
PV_API int pv_choir_synchronize(pv_choir *h);
/* Outputs [out_first, out_first + nout) of channels 0 .. nch-1, with pv_harmony_process's arguments and layout.  grains, voice_first and gains are HOST
 * tables.  Stateless.  Rejected with PV_ERR_ARGUMENT before any device work and with the output untouched: everything pv_harmony_process rejects, with the
 * grain rules above per voice (the message names voice and grain, the grain counted within its voice: a word of 2^27 or more or below 0, a step of
 * 1 .. 127 or above 512, a forward grain with D >= 2^30, any grain with D <= -2^30, a half length outside [2, max_period], centres out of order), and a
 * tile whose hull exceeds the span (the message names the tile and the first grain of its lowest voice).  nvoices > max_voices or nch > max_channels:
 * PV_ERR_CAPACITY.  Host pointers, synchronous, staged in pieces of whole tiles as pv_harmony_process. */
PV_API int pv_choir_process(pv_choir *h, const float *in, int64_t nin, int64_t in_stride, int32_t nch, const int32_t *grains, const int64_t *voice_first,
                            int32_t nvoices, const float *gains, float *out, int64_t out_first, int64_t nout, int64_t out_stride);
/* The same on DEVICE in / out pointers (grains, voice_first and gains stay host tables), asynchronous on the handle's stream. */
PV_API int pv_choir_process_device(pv_choir *h, const float *d_in, int64_t nin, int64_t in_stride, int32_t nch, const int32_t *grains,
                                   const int64_t *voice_first, int32_t nvoices, const float *gains, float *d_out, int64_t out_first, int64_t nout,
                                   int64_t out_stride);
/* Pure host code: pv_mirror_plan with pv_formant_plan's row warps.  warps == NULL: pv_mirror_plan's grains and output_len bit for bit; mirror == 0:
 * pv_formant_plan's.  With both, L and z of every grain come from pv_formant_plan's rule (s = floor(256 warps[record of A] + 1/2), the half length starts
 * from floor(period(A) / (s / 256.0) + 1/2)) and the direction, D and phi of a reuse from pv_mirror_plan's; a mirrored warped grain then reads about its own
 * mark: the analysis mark A at its centre, and (s / 256) L either side of it.  Marks, read position and output_len depend on neither.  Returns and refuses
 * as both planners do (mirror other than 0 or 1, a warp outside [1/2, 2]). */
PV_API int64_t pv_choir_plan(const pv_psola_params *p, const pv_epoch_params *e, const int32_t *records, int64_t nrec, const double *ratios,
                             const double *rates, const double *warps, const int32_t *epochs, int32_t mirror, int32_t *grains, int64_t capacity,
                             int64_t *output_len);

/* ---- per-take plans on the overlap-add path: one call plays K independently planned takes of different lengths (a separate handle) ---- */
/* A take is one monophonic recording with its own plan: its own input, far-grain table, length and output range.  (It is not a voice of pv_harmony,
 * a differently shifted copy of one input, and not a channel, a row that shares a plan.)  For every take k, channel c and n in
 * [out_first, out_first + nout), out[c * out_stride + n - out_first] is exactly what
 *     pv_tsm_process(h', in, nin, in_stride, nch, grains, ngrains, out, out_first, nout, out_stride)
 * writes for the take alone, h' a pv_tsm handle of the same (max_period, max_rate): the same bits.  Tiles of 1024 count from each take's own out_first,
 * and the span rule, and so which takes are refused, is pv_tsm_process's per take.  The order of every sum is a function of (g, i) alone: a take given as
 * two takes [0, a) and [a, n) that share `in` and write adjacent outputs gives the bits of one.  Takes may share an input (two plans on one recording:
 * a double-track); no two output rows of a call may overlap.  nch is common to the call.
 * The tiles of all takes go out in at most four launches, grouped by how many workgroups of their source range fit the LDS of a compute unit, so that
 * one take at a high rate does not lower the occupancy of the others (DESIGN.md "Takes"). */
typedef struct pv_take {
    const float   *in;          /* channel c at in + c*in_stride, nin samples (host or device, as the entry point says)              */
    int64_t        nin, in_stride;
    const int32_t *grains;      /* this take's far grains {t, w, D, L}, HOST, pv_tsm_process's rules word for word                   */
    int64_t        ngrains;
    float         *out;         /* channel c at out + c*out_stride; out[0] is output out_first                                       */
    int64_t        out_first, nout, out_stride;
} pv_take;

typedef struct pv_takes_config {
    int32_t struct_size;     /* sizeof(pv_takes_config) as the caller compiled it (PV_TAKES_CONFIG_INIT sets it)                  */
    int32_t max_period;      /* the largest half length L a take may pass, 2 .. 4096                                             */
    int32_t max_rate;        /* 1 .. 4: sizes the span, as pv_tsm_config                                                         */
    int32_t max_channels;    /* channels per call (0 => 1), at most 65535                                                        */
    int32_t max_outputs;     /* host-pointer calls: staging size in outputs (0 => 65536), rounded up to whole tiles of 1024       */
    int32_t device_id;       /* HIP device ordinal                                                                               */
    int32_t flags;           /* must be 0                                                                                        */
} pv_takes_config;
#define PV_TAKES_CONFIG_INIT { (int32_t)sizeof(pv_takes_config), 0, 0, 0, 0, 0, 0 }

typedef struct pv_takes pv_takes;

/* Config errors are returned before any device is touched, PV_ERR_UNSUPPORTED where pv_tsm_create returns it; failures are readable through
 * pv_takes_last_error(NULL).  There is no limit on the takes of a call to configure: the per-take device records grow on demand. */
PV_API int pv_takes_create(const pv_takes_config *cfg, pv_takes **out);
PV_API int pv_takes_destroy(pv_takes *h);
PV_API const char *pv_takes_last_error(const pv_takes *h);
/* Use an externally owned hipStream_t; NULL => the handle's own stream. */
PV_API int pv_takes_set_stream(pv_takes *h, void *hip_stream);
PV_API int pv_takes_synchronize(pv_takes *h);
/* ntakes takes of nch channels each, HOST in / out pointers, synchronous.  Everything is validated for all takes before any device work, and a refused
 * call leaves every take's output untouched.  PV_ERR_ARGUMENT: everything pv_tsm_process rejects, per take (the message names the take and the grain,
 * the grain counted within its take); ntakes < 0 or > 65536; a null takes with ntakes > 0; outputs that together reach 2^30 or more than 2^27 grains
 * together; two output rows, over all takes and channels, that overlap (the message names both takes).  nch > max_channels: PV_ERR_CAPACITY.
 * ntakes == 0, nch == 0 or every nout == 0: PV_OK, nothing queued.  A take with nout == 0 or ngrains == 0 is legal; outputs no grain covers are +0.
 * Staged in pieces: a piece is a run of consecutive tiles in take order with at most max_outputs outputs, and stages per take the input range its
 * tiles read. */
PV_API int pv_takes_process(pv_takes *h, const pv_take *takes, int32_t ntakes, int32_t nch);
/* The same with DEVICE in / out pointers in every take (takes and grains stay host tables), asynchronous on the handle's stream: one table upload and at
 * most four launches. */
PV_API int pv_takes_process_device(pv_takes *h, const pv_take *takes, int32_t ntakes, int32_t nch);
/* Pure host code: the tile walk the process calls run on.  cfg is validated as pv_takes_create validates it and used for max_period and max_rate only;
 * the takes are validated as the process calls validate them, except that in and out are never looked at and the overlap check is left out.  Per tile,
 * in take order and within a take in tile order, eight int32 {take, first, g_first, g_end, src0, src_count, cls, 0}: first is the tile's first output
 * relative to the take's out_first, g_first and g_end count within the take's own table, src0 and src_count are pv_tsm_process's source range of the
 * tile, and cls = min of 4 and 163840 div the LDS bytes of a launch that stages s samples, s = max of 128 and src_count rounded up to 64, is the
 * tile's occupancy class, always 1 .. 4: where the rounded s would not fit the LDS at all, s is src_count itself and cls is 1.  Returns the number of tiles and writes at most `capacity` of them; -PV_ERR_* on failure, with the message in
 * pv_takes_last_error(NULL): nothing is written then, except that the records before a tile beyond the span may have been. */
PV_API int64_t pv_takes_tiles(const pv_takes_config *cfg, const pv_take *takes, int32_t ntakes, int32_t *tiles, int64_t capacity);

/* ---- pitch contour tracking: several candidate periods per frame (a separate handle) and the cheapest path through them ------------------- */
/* pv_f0_track decides every frame alone, so a frame whose fundamental is weak reads an octave up.  Here a frame keeps K candidates and a path search
 * chooses among them under a cost for jumping and for switching voicing.  The path's output is f0 records (four int32 {tau, c(tau - 1), c(tau),
 * c(tau + 1)}, tau < 0 for an unvoiced frame, zeros for an empty one): pv_f0_period and every planner take it as they take pv_f0_track's.
 * Candidates.  Frame geometry, the scale, d(tau), cum(tau) and c(tau) for tau = 0 .. max_lag are exactly pv_f0_track's, with the same limits.  A lag tau
 * in [min_lag, max_lag - 1] is a dip when c(tau) < c(tau - 1) and c(tau) <= c(tau + 1); its key is ((c(tau) + (bias tau) div max_lag) << 16) | tau.  The
 * frame's K candidates are the K dips of smallest key, in key order: slot k = {tau, c(tau - 1), c(tau), c(tau + 1)}, {0, 0, 0, 0} beyond the number of
 * dips and in every slot of a silent frame or of one with a non-finite sample.  bias is per call, in [0, 16384], in units of 2^-14 over the whole lag
 * range: c is normalised by a cumulative mean, so under noise the dips at multiples of the period come out slightly deeper than the one at the period,
 * and the bias puts the shortest first (DESIGN.md "Pitch contour").  Every value is an exact integer function of the frame's samples. */
typedef struct pv_contour_config {
    int32_t struct_size;     /* sizeof(pv_contour_config) as the caller compiled it (PV_CONTOUR_CONFIG_INIT sets it)              */
    int32_t window;          /* W, the samples summed per lag                                                                    */
    int32_t hop;             /* samples between frames                                                                           */
    int32_t min_lag;         /* the shortest period looked for                                                                   */
    int32_t max_lag;         /* the lags computed; the longest period looked for is max_lag - 1                                  */
    int32_t candidates;      /* K, the slots per frame, 1 .. 8 (0 => 8)                                                          */
    int32_t max_channels;    /* channels per call (0 => 1), at most 65535                                                        */
    int32_t max_frames;      /* host-pointer calls: staging size in frames (0 => 256); longer calls go in pieces                 */
    int32_t device_id;       /* HIP device ordinal                                                                               */
    int32_t flags;           /* must be 0                                                                                        */
} pv_contour_config;
#define PV_CONTOUR_CONFIG_INIT { (int32_t)sizeof(pv_contour_config), 0, 0, 0, 0, 0, 0, 0, 0, 0 }

typedef struct pv_contour pv_contour;

/* Config errors are returned before any device is touched; failures are readable through pv_contour_last_error(NULL). */
PV_API int pv_contour_create(const pv_contour_config *cfg, pv_contour **out);
PV_API int pv_contour_destroy(pv_contour *h);
PV_API const char *pv_contour_last_error(const pv_contour *h);
/* Use an externally owned hipStream_t; NULL => the handle's own stream. */
PV_API int pv_contour_set_stream(pv_contour *h, void *hip_stream);
PV_API int pv_contour_synchronize(pv_contour *h);
/* nframes frames of channels 0 .. nch-1: channel c reads in[c*in_stride .. + (nframes - 1) hop + W + max_lag) and writes the K slots of frame m to
 * candidates[4 K (c*cand_stride + m) ..): cand_stride counts frames.  Rejected with PV_ERR_ARGUMENT before any device work and with the table untouched:
 * a null buffer, a negative count, a bias outside [0, 16384] and, with nch > 1, strides below what a channel reads and writes.  nch > max_channels:
 * PV_ERR_CAPACITY.  Host pointers, synchronous, staged in pieces of max_frames. */
PV_API int pv_contour_track(pv_contour *h, const float *in, int32_t nch, int64_t nframes, int64_t in_stride, int32_t bias, int32_t *candidates,
                            int64_t cand_stride);
/* The same on DEVICE in / candidates pointers (candidates 16-byte aligned: a slot is one store), asynchronous on the handle's stream. */
PV_API int pv_contour_track_device(pv_contour *h, const float *d_in, int32_t nch, int64_t nframes, int64_t in_stride, int32_t bias, int32_t *d_candidates,
                                   int64_t cand_stride);

/* Pure host code, integers only.  The cheapest path through the table of ONE channel: candidates holds nrec frames of K = p->candidates slots.  The
 * states of frame m are its occupied slots (tau > 0) and the unvoiced state, index K.  Costs in int64:
 *   o_m(s)      slot s: min(c0, 16384) + (bias tau) div max_lag.  Unvoiced: unvoiced_cost when slot 0 of the frame is occupied, else 0.
 *   t(a -> b)   0 from unvoiced to unvoiced, voicing_cost between unvoiced and voiced either way, (2 jump_cost |tau_b - tau_a|) div (tau_a + tau_b)
 *               between two slots: an octave either way costs two thirds of jump_cost.
 *   D_0(s) = o_0(s), D_m(s) = o_m(s) + min_a (D_(m-1)(a) + t(a -> s)), the tie to the lowest a; the last state is the first argmin of D_(nrec-1).
 * records[4 m ..) is the slot itself for a voiced state, slot 0 with tau negated for the unvoiced state, and zeros where slot 0 is empty; states, when
 * not NULL, gets the state index per frame.  With the ranges below the largest intermediate is under 2^38 per frame and under 2^62 over 2^31 - 1
 * frames.  PV_ERR_ARGUMENT with records untouched: a null pointer with nrec > 0, nrec negative or above 2^31 - 1, a parameter out of range, or a table
 * with tau < 0, tau > 65535 or a negative c value.  nrec = 0 is PV_OK.  The back pointers (nrec (K + 1) bytes) are allocated inside: PV_ERR_DEVICE
 * when the host is out of memory, as the create functions. */
typedef struct pv_contour_params {
    int32_t struct_size;     /* sizeof(pv_contour_params) as the caller compiled it (PV_CONTOUR_PARAMS_INIT sets it)              */
    int32_t candidates;      /* K of the table, 1 .. 8                                                                           */
    int32_t max_lag;         /* the tracker's, 3 .. 4096                                                                         */
    int32_t bias;            /* 0 .. 16384, normally the bias the table was made with                                            */
    int32_t unvoiced_cost;   /* 1 .. 16384: what pv_f0_track's threshold is to a single frame                                    */
    int32_t voicing_cost;    /* 0 .. 2^20                                                                                        */
    int32_t jump_cost;       /* 0 .. 2^20                                                                                        */
    int32_t reserved;        /* must be 0                                                                                        */
} pv_contour_params;
#define PV_CONTOUR_PARAMS_INIT { (int32_t)sizeof(pv_contour_params), 8, 0, 1024, 2458, 2458, 16384, 0 }
PV_API int pv_contour_path(const pv_contour_params *p, const int32_t *candidates, int64_t nrec, int32_t *records, int32_t *states);

#ifdef __cplusplus
}
#endif
#endif /* PHAZE_AMD_H */
