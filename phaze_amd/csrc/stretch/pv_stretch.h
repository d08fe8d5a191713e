// pv_stretch.h -- launch interface of the time-stretch kernels (internal; the public ABI is include/phaze_amd.h, pv_stretch_*).
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>

// Per-channel state slot, in floats / u32 words: hist[N - ha] | acc[N - hs] | phi[H] | psi[H]  (H = N/2 + 1).
inline long pv_stretch_state_stride(int N, int ha, int hs) { return (long)(N - ha) + (N - hs) + 2L * (N / 2 + 1); }

struct PvStretchParams {
    const float *in;          // channel c at in + c * in_stride: nframes * ha samples (with pos: pos[c * pos_stride + nframes] samples)
    float *out;               // channel c at out + c * out_stride: nframes * hs samples
    long in_stride, out_stride;
    int nframes, nch;
    int ha, hs;               // ha: the analysis hop, or with pos the floor of the scheduled hops (hist holds N - ha samples either way)
    int F;                    // frames per chain (>= halo + 1 whenever there is more than one chain)
    int nchains;              // chains per channel
    int halo;                 // (N - 1) / hs: earlier frames that overlap a frame's first output sample
    float ola_scale;          // hs / N = 1 / R_s
    const float *state_in;    // [nch][state_stride] carried state in
    float *state_out;         // [nch][state_stride] carried state out (the host copies it back behind the launch)
    long state_stride;
    unsigned *sums;           // [groups][nchains][2][H]: pass A writes {main, halo} advance sums, the scan turns the halo slot into pass B's start carry
    const double2 *tw64;      // exp(-2 pi j k / N), k in [0, N)
    const float2 *tw32;
    const float *hann;        // periodic Hann, f32, N values
    const long long *pos;     // variable tempo: [rows][nframes + 1] input consumed before frame m, S[0] = 0, S[m + 1] - S[m] = frame m's hop in [ha, N];
                              // frame m's window is stream[S[m + 1] - ha, + N).  nullptr: S[m] = m ha (the fixed-hop kernels)
    long pos_stride;          // int64 per row of pos (0: one row shared by every channel)
};

bool pv_stretch_supported(int log2n);                     // N = 256 .. 8192
size_t pv_stretch_lds_bytes(int log2n, bool pass_b);
int pv_stretch_threads();
// pass A + scan + pass B on `st`; the caller then copies state_out back into its state.  G = 1: every slot on its own; G >= 2: linked groups of G
// consecutive slots, p.nch a multiple of G (pass A and the scan run per group, pass B per channel).  p.sums holds [nch / G][nchains][2][H].
// rst != nullptr: phase resets, psi := q at flagged frames (p.pos must be set).  rst holds int32 prefix counts of the flags, [rows][nframes + 1]
// (R[0] = 0, R[m + 1] - R[m] = frame m's flag), the row of slot c at rst + c * rst_stride (0: one row for every slot); a group reads the row of slot g G.
hipError_t pv_launch_stretch(int log2n, const PvStretchParams &p, int G, const int *rst, long rst_stride, hipStream_t st);
// onset strength (pv_onset_kernels.hip): counts[g * count_stride + m] for the nch / G groups of `in` (channel c at in + c * in_stride, nframes * ha
// samples), one workgroup per (chain of F frames, group); stateless
hipError_t pv_launch_onset_strength(int log2n, const float *in, long in_stride, int nch, int G, int nframes, int ha, int F, const double2 *tw64,
                                    const float *hann, int *counts, long count_stride, hipStream_t st);
// the f0 tracker (pv_f0_kernels.hip): records[(c * rec_stride + m) * 4 ..) = {lag, c(lag - 1), c(lag), c(lag + 1)} of frame m of channel c, which reads
// in[c * in_stride + m * hop, + W + max_lag); one workgroup per (frame, channel); stateless.  records is 16-byte aligned, rec_stride counts records
hipError_t pv_launch_f0(const float *in, long in_stride, int nch, int nframes, int W, int hop, int min_lag, int max_lag, int threshold, int *records,
                        long rec_stride, hipStream_t st);
size_t pv_f0_lds_bytes(int W, int max_lag);
