// pv_stretch_synth.inc -- pass B fragment (pv_stretch_device.h): every bin A[k] rotated by its peak's angle psi[P] - phi[P] (rotate), the fp32
// c2r inverse, Hann and overlap-add scaled by hs / N into ring[base ..] (mod N).  Included in place inside the frame loop; it uses the enclosing
// kernel's C = SC<LOG2N>, N, M, tid, p, inv_n, A, B (aliasing A), P, psi, phi, ring and base.  Ends with a barrier.
        // locking + c2r pre-pass: Z[k] = E + jD, Z[M-k] = conj E + j conj D, E = Y[k] + conj Y[M-k], D = W^-k (Y[k] - conj Y[M-k]) (Im of Y[0], Y[M] dropped)
        float2 zlo[C::PAIRS], zhi[C::PAIRS];
#pragma unroll
        for (int i = 0; i < C::PAIRS; i++) {
            const int k = tid + i * TPB;
            zlo[i] = zhi[i] = float2{0.0f, 0.0f};
            if (k == 0) {
                const float r0 = rotate(A[0], P[0], psi, phi).x, rM = rotate(A[M], P[M], psi, phi).x;
                zlo[i] = float2{r0 + rM, r0 - rM};
            } else if (k <= M / 2) {
                const float2 yk = rotate(A[k], P[k], psi, phi), yc = rotate(A[M - k], P[M - k], psi, phi);
                const float2 E{yk.x + yc.x, yk.y - yc.y};
                const float2 Dm{yk.x - yc.x, yk.y + yc.y};
                const float2 w = p.tw32[k];
                const float2 D{__fadd_rn(__fmul_rn(Dm.x, w.x), __fmul_rn(Dm.y, w.y)), __fsub_rn(__fmul_rn(Dm.y, w.x), __fmul_rn(Dm.x, w.y))};
                zlo[i] = float2{E.x - D.y, E.y + D.x};
                zhi[i] = float2{E.x + D.y, D.x - E.y};
            }
        }
        __syncthreads();
#pragma unroll
        for (int i = 0; i < C::PAIRS; i++) {
            const int k = tid + i * TPB;
            if (k <= M / 2) {
                B[k] = zlo[i];
                if (k != 0 && k != M - k) B[M - k] = zhi[i];
            }
        }
        __syncthreads();
        // inverse: radix-2 DIF, natural order in, bit-reversed out, fp32
#pragma unroll 1
        for (int s = M / 2; s >= 1; s >>= 1) {
            const int tws = N / (2 * s);
            for (int jj = tid; jj < M / 2; jj += TPB) {
                const int pos = jj & (s - 1);
                const int i0 = ((jj - pos) << 1) + pos, i1 = i0 + s;
                const float2 w = p.tw32[pos * tws];                  // conj(w) = exp(+2 pi j pos / 2s)
                const float2 a = B[i0], bb = B[i1];
                const float2 d{a.x - bb.x, a.y - bb.y};
                B[i0] = float2{a.x + bb.x, a.y + bb.y};
                B[i1] = float2{__fadd_rn(__fmul_rn(d.x, w.x), __fmul_rn(d.y, w.y)), __fsub_rn(__fmul_rn(d.y, w.x), __fmul_rn(d.x, w.y))};
            }
            __syncthreads();
        }
        // frame = Hann * f32(Re IDFT / N); ring += frame * hs / N
        for (int n = tid; n < M; n += TPB) {
            const float2 z = B[__brev((unsigned)n) >> (32 - C::LOGM)];
            const float x0 = __fmul_rn(__fmul_rn(z.x, inv_n), p.hann[2 * n]);
            const float x1 = __fmul_rn(__fmul_rn(z.y, inv_n), p.hann[2 * n + 1]);
            const int r0 = (base + 2 * n) & (N - 1), r1 = (base + 2 * n + 1) & (N - 1);
            ring[r0] = __fadd_rn(ring[r0], __fmul_rn(x0, p.ola_scale));
            ring[r1] = __fadd_rn(ring[r1], __fmul_rn(x1, p.ola_scale));
        }
        __syncthreads();
