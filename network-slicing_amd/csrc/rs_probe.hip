// rs_probe.hip -- TEST BUILD ONLY (#included by rs_api.hip inside #ifdef RS_DEV; libranslice.so has none of it).
//
// rs_dev_probe evaluates ONE arithmetic primitive of the parity argument per element on the device, so that
// tests/test_gpu_primitives.py can compare it with the oracle's value of the same primitive bit for bit: the deterministic
// elementary functions in the code shapes the kernels call them in (out of line, in line, the two-argument forms), the raw
// f64 operations they are built from, the Philox block and every stream draw, the pairwise sums across lanes and teams, and
// the two float32 chains of the reception test.  It calls the production device functions themselves.  One thread per
// element, no loop of its own; every lane of a wave runs to the end (the pairwise sums are wave-uniform code).
//
// Layout of `in` / `out` per op (n elements; "pairs" are row-major):
//   the unary f64 ops (RSP_EXP_OOL .. RSP_RINT but the three below)   in f64[n]   out f64[n]
//   RSP_EXP2_OOL, RSP_SIGMOID2                in f64[n]                      out f64[n][2]: thread i evaluates (in[i], in[n-1-i])
//   RSP_DIV                                   see below
//   params = {x0, k} for RSP_SIGMOID, RSP_SIGMOID2, RSP_INV_SIGMOID
//   RSP_DIV                                   in f64[2][n] (a, b)            out f64[n] = a / b
//   RSP_FMA                                   in f64[3][n] (a, b, c)         out f64[n] = fma(a, b, c)
//   RSP_PHILOX                                in u32[n][6] (c0..c3, k0, k1)  out u32[n][2]
//   RSP_UNIFORM .. RSP_NORMAL                 in u32[n][5] (key0, key1, slice, serial, ctr)   out f64[n][2] (value, ctr after)
//       params: exponential {scale}, integers {n}, normal {loc, scale}
//   RSP_WALKER                                in u32[n][6] (key0, key1, slice, serial, now, attempt), params = {T}   out i32[n][2]
//   RSP_MACRO_CELL                            in u32[n][5], params = {prop_A, prop_B}         out f64[n][2] (nominal SINR, ctr after)
//   RSP_LANE_PAIRWISE                         in i32[n][2] (length 0..256, offset) then f64[m], params = {m}   out f64[n]
//   RSP_TEAM_PAIRWISE                         in i32[n/8][2] per 8-lane team, then f64[m], params = {m}; n % 8 == 0   out f64[n/8]
//   RSP_FAST_SIGMOID                          in f32[n], params = {x0, k, nominal SINR}       out f32[n]
//   RSP_RX_DQ                                 in f64[n] (the draw u), params = {mcsA, mcsB}   out f32[n]

enum {
    RSP_EXP_OOL = 0, RSP_EXP_INLINE, RSP_EXP_NONPOS, RSP_EXP2_OOL, RSP_LOG_OOL, RSP_LOG_INLINE, RSP_LOG10, RSP_ACOS,
    RSP_SIGMOID, RSP_SIGMOID2, RSP_INV_SIGMOID, RSP_DIV, RSP_SQRT, RSP_RINT, RSP_FMA,
    RSP_PHILOX, RSP_UNIFORM, RSP_EXPONENTIAL, RSP_INTEGERS, RSP_PM1, RSP_NORMAL, RSP_WALKER, RSP_MACRO_CELL,
    RSP_LANE_PAIRWISE, RSP_TEAM_PAIRWISE, RSP_FAST_SIGMOID, RSP_RX_DQ, RSP_N_OPS
};

struct ProbeArgs {
    const void* in;
    void* out;
    int64_t n;
    const RsDev* D;   // RSP_MACRO_CELL (prop_A, prop_B), RSP_RX_DQ (rx_B, rx_invA)
    double p[4];
    float f[4];
};

template <int OP>
__global__ __launch_bounds__(256) void probe_kernel(ProbeArgs a) {
#if defined(__HIP_DEVICE_COMPILE__)  // (the out-of-line and two-argument forms exist in the device pass only: rs_embb.hip)
    const int64_t i = (int64_t)blockIdx.x * 256 + (int64_t)threadIdx.x;
    const bool live = i < a.n;
    const int64_t e = live ? i : 0;  // (a lane past the end re-reads element 0 and stores nothing)
    const double* in = (const double*)a.in;
    double* out = (double*)a.out;
    if constexpr (OP <= RSP_RINT && OP != RSP_EXP2_OOL && OP != RSP_SIGMOID2 && OP != RSP_DIV) {
        const double x = in[e];
        double y;
        if constexpr (OP == RSP_EXP_OOL) y = rs_exp_ool(x);
        if constexpr (OP == RSP_EXP_INLINE) y = rs_exp(x);
        if constexpr (OP == RSP_EXP_NONPOS) y = rs_exp_nonpos(x);
        if constexpr (OP == RSP_LOG_OOL) y = rs_log_ool(x);
        if constexpr (OP == RSP_LOG_INLINE) y = rs_log(x);
        if constexpr (OP == RSP_LOG10) y = rs_log10(x);
        if constexpr (OP == RSP_ACOS) y = rs_acos(x);
        if constexpr (OP == RSP_SIGMOID) y = rs_sigmoid(x, a.p[0], a.p[1]);
        if constexpr (OP == RSP_INV_SIGMOID) y = rs_inv_sigmoid(x, a.p[0], a.p[1]);
        if constexpr (OP == RSP_SQRT) y = RS_SQRT(x);
        if constexpr (OP == RSP_RINT) y = RS_RINT(x);
        if (live) out[i] = y;
    } else if constexpr (OP == RSP_EXP2_OOL || OP == RSP_SIGMOID2) {
        const double x1 = in[e], x2 = in[a.n - 1 - e];
        rs_d2 o;
        if constexpr (OP == RSP_EXP2_OOL) {
            rs_d2 t;
            t.x = x1;
            t.y = x2;
            o = rs_exp2_ool(t);
        } else {
            o = rs_sigmoid2(x1, x2, a.p[0], a.p[1]);
        }
        if (live) {
            out[2 * i] = o.x;
            out[2 * i + 1] = o.y;
        }
    } else if constexpr (OP == RSP_DIV) {
        const double y = in[e] / in[a.n + e];
        if (live) out[i] = y;
    } else if constexpr (OP == RSP_FMA) {
        const double y = RS_FMA(in[e], in[a.n + e], in[2 * a.n + e]);
        if (live) out[i] = y;
    } else if constexpr (OP == RSP_PHILOX) {
        const uint32_t* w = (const uint32_t*)a.in + 6 * e;
        uint32_t o0, o1;
        rs_philox4x32_10(w[0], w[1], w[2], w[3], w[4], w[5], &o0, &o1);
        if (live) {
            ((uint32_t*)a.out)[2 * i] = o0;
            ((uint32_t*)a.out)[2 * i + 1] = o1;
        }
    } else if constexpr (OP >= RSP_UNIFORM && OP <= RSP_NORMAL) {
        const uint32_t* w = (const uint32_t*)a.in + 5 * e;
        rs_stream st = {w[0], w[1], w[2], w[3], w[4]};
        double v;
        if constexpr (OP == RSP_UNIFORM) v = rs_stream_uniform(&st);
        if constexpr (OP == RSP_EXPONENTIAL) v = rs_stream_exponential(&st, a.p[0]);
        if constexpr (OP == RSP_INTEGERS) v = (double)rs_stream_integers(&st, (int64_t)a.p[0]);
        if constexpr (OP == RSP_PM1) v = (double)rs_stream_pm1(&st);
        if constexpr (OP == RSP_NORMAL) v = rs_stream_normal(&st, a.p[0], a.p[1]);
        if (live) {
            out[2 * i] = v;
            out[2 * i + 1] = (double)st.ctr;
        }
    } else if constexpr (OP == RSP_WALKER) {
        const uint32_t* w = (const uint32_t*)a.in + 6 * e;
        int findex, fstep;
        rs_walker_redraw(w[0], w[1], w[2], w[3], w[4], w[5], (int)a.p[0], &findex, &fstep);
        if (live) {
            ((int32_t*)a.out)[2 * i] = findex;
            ((int32_t*)a.out)[2 * i + 1] = fstep;
        }
    } else if constexpr (OP == RSP_MACRO_CELL) {
        const uint32_t* w = (const uint32_t*)a.in + 5 * e;
        const rs_stream st = {w[0], w[1], w[2], w[3], w[4]};
        const MacroCell mc = macro_cell_draw(a.D, st);
        if (live) {
            out[2 * i] = mc.x;
            out[2 * i + 1] = mc.y;
        }
    } else if constexpr (OP == RSP_LANE_PAIRWISE) {
        const int32_t* w = (const int32_t*)a.in + 2 * e;
        const double* vec = (const double*)((const int32_t*)a.in + 2 * a.n);
        const int len = live ? w[0] : 0;
        const double* __restrict__ colp = vec + (live ? w[1] : 0);
        const double s = lane_pairwise(len, len > 0, [&](int k) { return colp[k]; });
        if (live) out[i] = s;
    } else if constexpr (OP == RSP_TEAM_PAIRWISE) {
        const int64_t team = e >> 3;
        const int j = (int)(threadIdx.x & 7u);
        const int32_t* w = (const int32_t*)a.in + 2 * team;
        const double* vec = (const double*)((const int32_t*)a.in + 2 * (a.n >> 3));
        const int len = live ? w[0] : 0;
        const bool on = len > 0;
        const double* __restrict__ sp = vec + (on ? w[1] : 0);
        const double s = team_pairwise(len, j, on, [&](int i1, bool p1, int i2, bool p2) {
            rs_d2 o;
            o.x = p1 ? sp[i1] : 0.0;
            o.y = p2 ? sp[i2] : 0.0;
            return o;
        });
        if (live && j == 0) out[team] = s;
    } else if constexpr (OP == RSP_FAST_SIGMOID) {
        // (hi, c1, loc) as fast_team_sums / fast_wide_sums form them: nomx = nominal SINR - x0 in f64, c1 = RsDev.rx_c1
        const double nomx = a.p[2] - a.p[0];
        const float c1 = a.f[0];
        const float hi = (float)nomx, loc = (float)(nomx - (double)hi) * c1;
        const float y = fast_sigmoid(((const float*)a.in)[e], hi, c1, loc);
        if (live) ((float*)a.out)[i] = y;
    } else if constexpr (OP == RSP_RX_DQ) {
        const double u = in[e];
        const RsDev* D = a.D;
        const float lf = RS_RX_LF(u);
        const float dq = RS_RX_DQ(D, lf);
        if (live) ((float*)a.out)[i] = dq;
    }
#endif
}

extern "C" int rs_dev_probe(int device, int op, const void* in, void* out, int64_t n, const double* params) {
    if (op < 0 || op >= RSP_N_OPS || n <= 0 || n > ((int64_t)1 << 22) || !in || !out) return RS_EINVAL;
    ProbeArgs a;
    memset(&a, 0, sizeof a);
    a.n = n;
    for (int k = 0; k < 4; ++k) a.p[k] = params ? params[k] : 0.0;
    size_t in_bytes = 8 * (size_t)n, out_bytes = 8 * (size_t)n, in_pad = 0;
    bool needs_params = false;
    switch (op) {
        case RSP_SIGMOID: case RSP_INV_SIGMOID: needs_params = true; break;
        case RSP_EXP2_OOL: out_bytes = 16 * (size_t)n; break;
        case RSP_SIGMOID2: out_bytes = 16 * (size_t)n; needs_params = true; break;
        case RSP_DIV: in_bytes = 16 * (size_t)n; break;
        case RSP_FMA: in_bytes = 24 * (size_t)n; break;
        case RSP_PHILOX: in_bytes = 24 * (size_t)n; break;
        case RSP_WALKER: in_bytes = 24 * (size_t)n; needs_params = true; break;
        case RSP_UNIFORM: case RSP_PM1: in_bytes = 20 * (size_t)n; out_bytes = 16 * (size_t)n; break;
        case RSP_EXPONENTIAL: case RSP_INTEGERS: case RSP_NORMAL: case RSP_MACRO_CELL:
            in_bytes = 20 * (size_t)n;
            out_bytes = 16 * (size_t)n;
            needs_params = true;
            break;
        case RSP_LANE_PAIRWISE: case RSP_TEAM_PAIRWISE: needs_params = true; break;  // (sizes: below)
        case RSP_FAST_SIGMOID: in_bytes = out_bytes = 4 * (size_t)n; needs_params = true; break;
        case RSP_RX_DQ: out_bytes = 4 * (size_t)n; needs_params = true; break;
        default: break;
    }
    if (needs_params && !params) return RS_EINVAL;
    if (op == RSP_INTEGERS && !(a.p[0] >= 1.0 && a.p[0] <= 9.0e15)) return RS_EINVAL;
    if (op == RSP_WALKER && !(a.p[0] >= 1.0 && a.p[0] <= 2147483647.0)) return RS_EINVAL;
    if (op == RSP_LANE_PAIRWISE || op == RSP_TEAM_PAIRWISE) {
        // every (length, offset) must lie inside the shared vector: checked here, the kernel trusts them
        if (!(a.p[0] >= 1.0 && a.p[0] <= (double)(1 << 24))) return RS_EINVAL;
        const int64_t m = (int64_t)a.p[0];
        if (op == RSP_TEAM_PAIRWISE && (n & 7)) return RS_EINVAL;
        const int64_t rows = op == RSP_TEAM_PAIRWISE ? n >> 3 : n;
        const int32_t* w = (const int32_t*)in;
        for (int64_t r = 0; r < rows; ++r)
            if (w[2 * r] < 0 || w[2 * r] > 256 || w[2 * r + 1] < 0 || (int64_t)w[2 * r + 1] + w[2 * r] > m) return RS_EINVAL;
        in_pad = 64 * 8;  // lane_block fetches its remainder unmasked: a lane may read (never use) the element after its span
        in_bytes = 8 * (size_t)rows + 8 * (size_t)m;
        out_bytes = 8 * (size_t)rows;
    }
    // the float constants of the reception test come from rx_fast_setup itself, run on a scratch RsDev
    // (the developer knobs it reads, RANSLICE_RX_EXACT and RANSLICE_RX_BAND_SCALE, only move the bands, which the probe ignores)
    RsDev* hd = new RsDev();
    memset(hd, 0, sizeof *hd);
    if (op == RSP_FAST_SIGMOID || op == RSP_RX_DQ) {
        // RSP_FAST_SIGMOID: the curve (x0, k) in all three slots; RSP_RX_DQ: (A, B), with curves that keep A/k in range
        const bool fs = op == RSP_FAST_SIGMOID;
        hd->mcsA = fs ? a.p[1] : a.p[0];
        hd->mcsB = fs ? 0.0 : a.p[1];
        for (int m = 0; m < 3; ++m) {
            hd->mi_k[m] = fs ? a.p[1] : a.p[0];
            hd->mi_x0[m] = fs ? a.p[0] : 0.0;
        }
        double band0 = 0.0;
        rx_fast_setup(*hd, &band0);
        a.f[0] = hd->rx_c1[0];
        if (hd->rx_invA == 0.0f) {  // a configuration the reception test is switched off for
            delete hd;
            return RS_EINVAL;
        }
    } else if (op == RSP_MACRO_CELL) {
        hd->prop_A = a.p[0];
        hd->prop_B = a.p[1];
    }
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || device < 0 || device >= ndev || hipSetDevice(device) != hipSuccess) {
        delete hd;
        return RS_EHIP;
    }
    void *d_in = nullptr, *d_out = nullptr;
    RsDev* d_dev = nullptr;
    int rc = RS_EHIP;
    do {
        if (hipMalloc(&d_in, in_bytes + in_pad) != hipSuccess || hipMalloc(&d_out, out_bytes) != hipSuccess) break;
        if (in_pad && hipMemset((char*)d_in + in_bytes, 0, in_pad) != hipSuccess) break;
        if (hipMemcpy(d_in, in, in_bytes, hipMemcpyHostToDevice) != hipSuccess) break;
        if (hipMemset(d_out, 0, out_bytes) != hipSuccess) break;
        if (op == RSP_MACRO_CELL || op == RSP_RX_DQ) {
            if (hipMalloc((void**)&d_dev, sizeof(RsDev)) != hipSuccess ||
                hipMemcpy(d_dev, hd, sizeof(RsDev), hipMemcpyHostToDevice) != hipSuccess)
                break;
            a.D = d_dev;
        }
        a.in = d_in;
        a.out = d_out;
        const dim3 grid((unsigned)((n + 255) / 256)), block(256);
        switch (op) {
#define RSP_CASE(OP) case OP: hipLaunchKernelGGL(probe_kernel<OP>, grid, block, 0, 0, a); break;
            RSP_CASE(RSP_EXP_OOL) RSP_CASE(RSP_EXP_INLINE) RSP_CASE(RSP_EXP_NONPOS) RSP_CASE(RSP_EXP2_OOL) RSP_CASE(RSP_LOG_OOL)
            RSP_CASE(RSP_LOG_INLINE) RSP_CASE(RSP_LOG10) RSP_CASE(RSP_ACOS) RSP_CASE(RSP_SIGMOID) RSP_CASE(RSP_SIGMOID2)
            RSP_CASE(RSP_INV_SIGMOID) RSP_CASE(RSP_DIV) RSP_CASE(RSP_SQRT) RSP_CASE(RSP_RINT) RSP_CASE(RSP_FMA) RSP_CASE(RSP_PHILOX)
            RSP_CASE(RSP_UNIFORM) RSP_CASE(RSP_EXPONENTIAL) RSP_CASE(RSP_INTEGERS) RSP_CASE(RSP_PM1) RSP_CASE(RSP_NORMAL)
            RSP_CASE(RSP_WALKER) RSP_CASE(RSP_MACRO_CELL) RSP_CASE(RSP_LANE_PAIRWISE) RSP_CASE(RSP_TEAM_PAIRWISE)
            RSP_CASE(RSP_FAST_SIGMOID) RSP_CASE(RSP_RX_DQ)
#undef RSP_CASE
            default: break;
        }
        if (hipGetLastError() != hipSuccess) break;
        if (hipDeviceSynchronize() != hipSuccess) break;
        if (hipMemcpy(out, d_out, out_bytes, hipMemcpyDeviceToHost) != hipSuccess) break;
        rc = RS_OK;
    } while (0);
    delete hd;
    if (d_in) (void)hipFree(d_in);
    if (d_out) (void)hipFree(d_out);
    if (d_dev) (void)hipFree(d_dev);
    if (hipDeviceSynchronize() != hipSuccess) rc = RS_EHIP;
    return rc;
}
