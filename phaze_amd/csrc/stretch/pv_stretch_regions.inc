// pv_stretch_regions.inc -- pass B fragment (pv_stretch_device.h): findPeaks on mag[0 .. H), then P[k] := the peak whose region of influence
// holds bin k (shiftPeaks at f = 1), -1 when the frame has no peak.  Included in place inside the frame loop; it uses the enclosing kernel's
// C = SC<LOG2N>, H, tid, mag, P (aliasing mag) and scL / scF (TPB ints each).  Ends with a barrier.
        // findPeaks: strict maximum over +-2 bins, k in [2, H - 2)
        unsigned fl = 0;
#pragma unroll
        for (int i = 0; i < C::BINS; i++) {
            const int k = tid + i * TPB;
            if (k >= 2 && k < H - 2) {
                const float v = mag[k];
                const bool pk = !(mag[k - 1] >= v || mag[k - 2] >= v || mag[k + 1] >= v || mag[k + 2] >= v);
                fl |= (pk ? 1u : 0u) << i;
            }
        }
        __syncthreads();
#pragma unroll
        for (int i = 0; i < C::BINS; i++) {
            const int k = tid + i * TPB;
            if (k < H) P[k] = ((fl >> i) & 1u) ? k : NOPEAK;
        }
        __syncthreads();
        // regions: thread t walks the bins [t BINS, (t+1) BINS); the nearest peaks outside its segment come from a prefix max / suffix min over threads
        const int k0 = min(tid * C::BINS, H), k1 = min(k0 + C::BINS, H);
        {
            int lastp = -1, firstp = NOPEAK;
            for (int k = k0; k < k1; k++)
                if (P[k] != NOPEAK) { if (firstp == NOPEAK) firstp = k; lastp = k; }
            scL[tid] = lastp;
            scF[tid] = firstp;
        }
        __syncthreads();
#pragma unroll 1
        for (int off = 1; off < TPB; off <<= 1) {
            const int l = tid >= off ? scL[tid - off] : -1;
            const int f = tid + off < TPB ? scF[tid + off] : NOPEAK;
            __syncthreads();
            scL[tid] = max(scL[tid], l);
            scF[tid] = min(scF[tid], f);
            __syncthreads();
        }
        {
            int prev = tid > 0 ? scL[tid - 1] : -1;
            int next = tid + 1 < TPB ? scF[tid + 1] : NOPEAK;
            for (int k = k1 - 1; k >= k0; k--) {                      // P[k] := smallest peak >= k
                if (P[k] == k) next = k;
                P[k] = next;
            }
            for (int k = k0; k < k1; k++) {                           // region rule: between peaks a < b, bin k goes to b iff b - k <= floor((b - a) / 2)
                const int n = P[k];
                int r;
                if (n == k) { prev = k; r = k; }
                else if (prev < 0) r = n == NOPEAK ? -1 : n;
                else if (n == NOPEAK) r = prev;
                else r = (n - k <= (n - prev) / 2) ? n : prev;
                P[k] = r;
            }
        }
        __syncthreads();
