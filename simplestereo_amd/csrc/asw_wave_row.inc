// One image row of a wave kernel's window: the strip's e tile by LDS-DMA (one contiguous block of the TAD volume), the row's
// proximity weights, and the Lab values of the left and right tap columns into pixL / pixR.  Included ONCE, inside the loop over
// window rows, between the two asw_wave_sync() that separate it from the taps of the previous and of this row.  Text, not a
// function: see asw_wave_front.inc.
//
// Read by name:  i (window row), r (image row), A, lane, W, win, Se, x0, nLw, nRw, segL_lo, segR_lo, eT, pixL, pixR
//                (asw_wave_front.inc).
// Written:       proxv, declared by the kernel before the loop: lane j holds the proximity weight of tap column j as bits.
        {
            const unsigned char *const src = A.evol + (((size_t)(r - A.erow0)) * (size_t)A.evolW + x0) * Se;
            const int bytes = nLw * Se;
            for (int k = 0; k < bytes; k += 1024)
                if (k + lane * 16 < bytes)
                    __builtin_amdgcn_global_load_lds((const void *)(src + k + lane * 16),
                                                     (__attribute__((address_space(3))) void *)(eT + k), 16, 0, 0);
            proxv = __builtin_bit_cast(int, A.prox[i * win + min(lane, win - 1)]);   // lane j: proximity weight of tap column j
            const PixRec *const rowL = A.recL + (size_t)r * W, *const rowR = A.recR + (size_t)r * W;
            for (int k = lane; k < nLw + nRw; k += 64) {
                const bool isL = k < nLw;
                const int idx = isL ? k : k - nLw;
                const int col = (isL ? segL_lo : segR_lo) + idx;
                // a tap column outside the image gets L = +inf: its colour distance is +inf, exp2(-inf) = +0 and the
                // weight is exactly the +0 the other kernels produce with a mask, without an instruction for it
                float4 v = make_float4(__builtin_inff(), 0.f, 0.f, 0.f);
                if ((unsigned)col < (unsigned)W) {
                    const PixRec q = (isL ? rowL : rowR)[col];
                    v = make_float4(q.L, q.a, q.b, 0.f);
                }
                (isL ? pixL : pixR)[idx] = v;
            }
        }
