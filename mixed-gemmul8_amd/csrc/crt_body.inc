// crt_body.inc -- the body of crt_kernel (crt.hip), included by it and by its strided-batched form so that both
// run the same statements on `CrtArgs a`; template parameters OT, NUMM1, N, KARA, R, PFC are the including kernel's.
    static_assert(R == CRT_ROWS || R == 4, "rows per lane: 8 or 4");
    using W = RowWord<R>;
    using E = typename OutElem<OT>::T;
    constexpr int EPV = 16 / sizeof(E);  // elements per 16-byte vector
    __shared__ E buf[4][64 * R];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const size_t wrow0 = ((size_t)blockIdx.x * 256 + wv * 64) * R;
    if (wrow0 >= a.m) return;  // whole wave beyond the last row (no block-level sync below)
    const size_t r0 = wrow0 + (size_t)lane * R;
    const int nr = r0 >= a.m ? 0 : (a.m - r0 >= R ? R : (int)(a.m - r0));
    const bool plain_ab = a.ar == 1.0 && a.ai == 0.0 && a.br == 0.0 && a.bi == 0.0;
    // C is not read at beta = 0 (BLAS), except by the reference's _ab kernels (reference-epilogue mode)
    const bool zero_beta = a.br == 0.0 && a.bi == 0.0 && !(a.ref_epi && !(a.ar == 1.0 && a.ai == 0.0));
    int16_t sa[R];
#pragma unroll
    for (int e = 0; e < R; ++e) sa[e] = e < nr ? a.sftA[r0 + e] : 0;
    E *wb = buf[wv];
    // real outputs with several columns per block (PF): the next column's residue words are loaded before this
    // column's CRT, so they are in flight under its arithmetic and stores
    constexpr bool PF = PFC && !KARA && OT < 2;
    W wpf[PF ? N : 1];
    if constexpr (PF) {
        if (nr > 0 && blockIdx.y < a.n) load_rows<N>(a, blockIdx.y * a.ldr + r0, nr == R, nr, wpf);
    }
    for (size_t col = blockIdx.y; col < a.n; col += gridDim.y) {
        const int sB = a.sftB[col];
        if (nr > 0) {
            W w[N], wi[N];
            const size_t off = col * a.ldr + r0;
            if constexpr (PF) {
#pragma unroll
                for (unsigned i = 0; i < N; ++i) w[i] = wpf[i];
                const size_t nxt = col + gridDim.y;
                if (nxt < a.n) load_rows<N>(a, nxt * a.ldr + r0, nr == R, nr, wpf);
            }
            if constexpr (KARA) {
                // real parts from P1, P2 first, then the imaginary parts with P3: two sub-planes' words
                // live at a time instead of three (occupancy; the residues are the same bytes)
                W w1[N], w2[N];
                load_rows<N>(a, off, nr == R, nr, w1);
                load_rows<N>(a, off + a.sub, nr == R, nr, w2);
                kara_pair_words<N>(w1, w2, w, wi, std::make_integer_sequence<unsigned, N>{});
                // P3's loads go out after that (an opaque dependency on the last combined word keeps the
                // compiler from merging them with P1's and P2's), in flight under the real parts
                size_t off3 = off + 2 * a.sub;
                asm volatile("" : "+v"(off3) : "v"(wi[N - 1]));
                W w3[N];
                load_rows<N>(a, off3, nr == R, nr, w3);
                if constexpr (OZ2_CRT_MODOUTER) {
                    double v[R];
                    crt_rows_const<N, NUMM1, R>(w, v, std::make_integer_sequence<unsigned, N>{});
#pragma unroll
                    for (int e = 0; e < R; ++e) {
                        const double vr = scalbn(v[e], (int)sa[e] + sB);
                        if constexpr (OT == 2) wb[crt_slot<E, R>(lane, e)].x = vr;
                        else wb[crt_slot<E, R>(lane, e)].x = __double2float_rn(vr);
                    }
                } else {
#pragma unroll
                    for (int e = 0; e < R; ++e) {
                        uint8_t r[N];
#pragma unroll
                        for (unsigned i = 0; i < N; ++i) r[i] = (uint8_t)(w[i] >> (8 * e));
                        const double vr = scalbn(crt_value_const<N, NUMM1>(r, std::make_integer_sequence<unsigned, N>{}),
                                                 (int)sa[e] + sB);
                        if constexpr (OT == 2) wb[crt_slot<E, R>(lane, e)].x = vr;
                        else wb[crt_slot<E, R>(lane, e)].x = __double2float_rn(vr);
                    }
                }
                asm volatile("" ::: "memory");  // the real parts go to LDS now (no merging with the imaginary ones)
                kara_sub_words<N>(w3, wi, std::make_integer_sequence<unsigned, N>{});
                if constexpr (OZ2_CRT_MODOUTER) {
                    double v[R];
                    crt_rows_const<N, NUMM1, R>(wi, v, std::make_integer_sequence<unsigned, N>{});
#pragma unroll
                    for (int e = 0; e < R; ++e) {
                        const double vi = scalbn(v[e], (int)sa[e] + sB);
                        if constexpr (OT == 2) wb[crt_slot<E, R>(lane, e)].y = vi;
                        else wb[crt_slot<E, R>(lane, e)].y = __double2float_rn(vi);
                    }
                } else {
#pragma unroll
                    for (int e = 0; e < R; ++e) {
                        uint8_t r[N];
#pragma unroll
                        for (unsigned i = 0; i < N; ++i) r[i] = (uint8_t)(wi[i] >> (8 * e));
                        const double vi = scalbn(crt_value_const<N, NUMM1>(r, std::make_integer_sequence<unsigned, N>{}),
                                                 (int)sa[e] + sB);
                        if constexpr (OT == 2) wb[crt_slot<E, R>(lane, e)].y = vi;
                        else wb[crt_slot<E, R>(lane, e)].y = __double2float_rn(vi);
                    }
                }
            } else if constexpr (!PF) {
                load_rows<N>(a, off, nr == R, nr, w);
                if (OT >= 2) load_rows<N>(a, off + a.imag_off, nr == R && (a.imag_off & 7) == 0, nr, wi);
            }
            constexpr bool MO = OZ2_CRT_MODOUTER_ALL || N >= OZ2_CRT_MODOUTER_MIN_N;
            if constexpr (!KARA && MO) {
                double vr[R], vi[R];
                crt_rows_const<N, NUMM1, R>(w, vr, std::make_integer_sequence<unsigned, N>{});
                if constexpr (OT >= 2) crt_rows_const<N, NUMM1, R>(wi, vi, std::make_integer_sequence<unsigned, N>{});
#pragma unroll
                for (int e = 0; e < R; ++e) {
                    const int sft = (int)sa[e] + sB;
                    const double x = scalbn(vr[e], sft);
                    if constexpr (OT == 0) wb[crt_slot<E, R>(lane, e)] = x;
                    else if constexpr (OT == 1) wb[crt_slot<E, R>(lane, e)] = __double2float_rn(x);
                    else if constexpr (OT == 2) wb[crt_slot<E, R>(lane, e)] = make_double2(x, scalbn(vi[e], sft));
                    else wb[crt_slot<E, R>(lane, e)] = make_float2(__double2float_rn(x), __double2float_rn(scalbn(vi[e], sft)));
                }
            }
#pragma unroll
            for (int e = 0; e < (KARA || MO ? 0 : R); ++e) {
                uint8_t r[N];
#pragma unroll
                for (unsigned i = 0; i < N; ++i) r[i] = (uint8_t)(w[i] >> (8 * e));
                const int sft = (int)sa[e] + sB;
                const double vr = scalbn(crt_value_const<N, NUMM1>(r, std::make_integer_sequence<unsigned, N>{}), sft);
                if constexpr (OT == 0) {
                    wb[crt_slot<E, R>(lane, e)] = vr;
                } else if constexpr (OT == 1) {
                    wb[crt_slot<E, R>(lane, e)] = __double2float_rn(vr);
                } else {
#pragma unroll
                    for (unsigned i = 0; i < N; ++i) r[i] = (uint8_t)(wi[i] >> (8 * e));
                    const double vi = scalbn(crt_value_const<N, NUMM1>(r, std::make_integer_sequence<unsigned, N>{}), sft);
                    if constexpr (OT == 2) wb[crt_slot<E, R>(lane, e)] = make_double2(vr, vi);
                    else wb[crt_slot<E, R>(lane, e)] = make_float2(__double2float_rn(vr), __double2float_rn(vi));
                }
            }
        }
        wave_sync();
        E *Cc = static_cast<E *>(a.C) + col * a.ldc + wrow0;
        const bool vec_ok = (reinterpret_cast<uintptr_t>(Cc) & 15) == 0;
#pragma unroll
        for (int j = 0; j < R / EPV; ++j) {
            const int idx = j * 64 * EPV + lane * EPV;
            E v[EPV];
            *reinterpret_cast<int4 *>(v) = *reinterpret_cast<const int4 *>(wb + crt_slot<E, R>(idx / R, idx % R));
            if (vec_ok && wrow0 + idx + EPV <= a.m) {
                if (!plain_ab) {
                    E c[EPV];
                    if (zero_beta) {
#pragma unroll
                        for (int q = 0; q < EPV; ++q) c[q] = E{};
                    } else {
                        *reinterpret_cast<int4 *>(c) = *reinterpret_cast<const int4 *>(Cc + idx);
                    }
#pragma unroll
                    for (int q = 0; q < EPV; ++q) v[q] = BlasEpi<OT>::template f<NUMM1>(v[q], c[q], a);
                }
                if (OZ2_CRT_NT & 2) {
                    typedef int i4v __attribute__((ext_vector_type(4)));
                    __builtin_nontemporal_store(*reinterpret_cast<const i4v *>(v), reinterpret_cast<i4v *>(Cc + idx));
                } else {
                    *reinterpret_cast<int4 *>(Cc + idx) = *reinterpret_cast<const int4 *>(v);
                }
            } else {
#pragma unroll
                for (int q = 0; q < EPV; ++q) {
                    if (wrow0 + idx + q < a.m) {
                        E x = v[q];
                        if (!plain_ab) x = BlasEpi<OT>::template f<NUMM1>(x, zero_beta ? E{} : Cc[idx + q], a);
                        Cc[idx + q] = x;
                    }
                }
            }
        }
        wave_sync();
    }
