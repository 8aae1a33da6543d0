/*
 * rf_oracle_body.inc -- tracer restatement, instantiated twice by rf_oracle.c
 * (REAL=float: the pinned fp32 arithmetic with the fp16 face table; REAL=double: validation twin).
 * TEST INFRASTRUCTURE ONLY -- see the header of rf_oracle.c.
 */

typedef struct {
    int sh_degree;
    int attr_dim;               /* A = 1 + 3*(d+1)^2                                      */
    rfo_settings settings;
    uint32_t num_points;
    const REAL *points;         /* [N,3]                                                  */
    const REAL *attributes;     /* [N,A]  row = [3B SH | density]                         */
    const uint32_t *adj;        /* [E]                                                    */
    const uint32_t *offsets;    /* [N+1]                                                  */
    const uint16_t *diff;       /* [E,4] half (REAL=float only)                           */
} SUF(foam_t);

/* scatter-add; atomic when several OpenMP threads share the accumulator */
static inline void SUF(acc)(REAL *dst, REAL v, int atomic) {
    if (atomic) {
#pragma omp atomic
        *dst += v;
    } else {
        *dst += v;
    }
}

/* Where a backward walk adds its gradients: the output arrays directly (one thread), with atomics (contribution of the
 * forward), or -- float instance, several threads -- a thread-local write-combining table of rows [point gradient |
 * attribute gradient | point error] keyed by cell (rf_oracle.c: rfo_wc_t), merged into the output arrays when it fills
 * and at the end: no atomic in the walk (BASELINE.md section 3: "thread-local gradient buffers reduced at the end"). */
typedef struct {
    REAL *pg, *ag, *pe;
    int atomic;
    void *wc;
    /* optional magnitude shadow (rfo_trace_backward_mag): mag_base mirrors, element for element, the block of REALs that
     * starts at base -- the output arrays laid out [pg | ag | pe], or the rows of the write-combining table -- and receives
     * |v| in double for every v added there.  NULL: no shadow, and nothing below touches it. */
    const REAL *base;
    double *mag_base;
} SUF(sink_t);

/* a gradient add: the value as ever, and its absolute value into the shadow of the same element when there is one */
static inline void SUF(sink_add)(const SUF(sink_t) *k, REAL *dst, REAL v, int atomic) {
    SUF(acc)(dst, v, atomic);
    if (k->mag_base) {
        double *m = k->mag_base + (dst - k->base);
        const double a = fabs((double)v);
        if (atomic) {
#pragma omp atomic
            *m += a;
        } else {
            *m += a;
        }
    }
}

static inline REAL *SUF(sink_row)(const SUF(sink_t) *k, uint32_t cell, int A, REAL **pg, REAL **pe) {
#if RFO_HALF_FACES
    if (k->wc) {
        float *row = rfo_wc_row((rfo_wc_t *)k->wc, cell);
        *pg = row;
        *pe = row + 3 + A;
        return row + 3;
    }
#endif
    *pg = k->pg + 3 * (size_t)cell;
    *pe = k->pe ? k->pe + cell : NULL;
    return k->ag + (size_t)cell * A;
}

static inline REAL SUF(dot3)(const REAL *a, const REAL *b) {
    return R_FMA(a[0], b[0], R_FMA(a[1], b[1], a[2] * b[2]));
}

/* ray.direction /= ray.direction.norm()                      src/tracing/pipeline.cu:40,162 */
static inline void SUF(normalize3)(REAL *d) {
    REAL n = R_SQRT(SUF(dot3)(d, d));
    d[0] = d[0] / n;
    d[1] = d[1] / n;
    d[2] = d[2] / n;
}

/* sh_coefficients<degree>                                    src/tracing/sh_utils.cuh:8-70 */
static void SUF(sh_basis)(int degree, const REAL *dir, REAL *sh) {
    const REAL C0 = (REAL)0.28209479177387814f;
    const REAL C1 = (REAL)0.4886025119029199f;
    const REAL C2[5] = {(REAL)1.0925484305920792f, (REAL)-1.0925484305920792f,
                        (REAL)0.31539156525252005f, (REAL)-1.0925484305920792f,
                        (REAL)0.5462742152960396f};
    const REAL C3[7] = {(REAL)-0.5900435899266435f, (REAL)2.890611442640554f,
                        (REAL)-0.4570457994644658f, (REAL)0.3731763325901154f,
                        (REAL)-0.4570457994644658f, (REAL)1.445305721320277f,
                        (REAL)-0.5900435899266435f};
    REAL x = dir[0], y = dir[1], z = dir[2];
    sh[0] = C0;
    if (degree > 0) {
        sh[1] = -C1 * y;
        sh[2] = C1 * z;
        sh[3] = -C1 * x;
    }
    REAL xx = x * x, yy = y * y, zz = z * z;
    REAL xy = x * y, yz = y * z, xz = x * z;
    if (degree > 1) {
        sh[4] = C2[0] * xy;
        sh[5] = C2[1] * yz;
        sh[6] = C2[2] * (((REAL)2 * zz - xx) - yy);
        sh[7] = C2[3] * xz;
        sh[8] = C2[4] * (xx - yy);
    }
    if (degree > 2) {
        sh[9] = (C3[0] * y) * R_FMA((REAL)3, xx, -yy);
        sh[10] = (C3[1] * xy) * z;
        sh[11] = (C3[2] * y) * (((REAL)4 * zz - xx) - yy);
        sh[12] = (C3[3] * z) * R_FMA((REAL)-3, yy, R_FMA((REAL)-3, xx, (REAL)2 * zz));
        sh[13] = (C3[4] * x) * (((REAL)4 * zz - xx) - yy);
        sh[14] = (C3[5] * z) * (xx - yy);
        sh[15] = (C3[6] * x) * R_FMA((REAL)-3, yy, xx);
    }
}

/* load_attributes lambda + load_sh_as_rgb     src/tracing/pipeline.cu:47-55, sh_utils.cuh:72-83 */
static inline void SUF(load_attributes)(const SUF(foam_t) *fm, const REAL *sh, uint32_t cell,
                                        REAL *rgb, REAL *s) {
    const REAL *row = fm->attributes + (size_t)cell * fm->attr_dim;
    *s = row[fm->attr_dim - 1];
    if (*s > (REAL)1e-6f) {
        REAL c[3] = {(REAL)0.5, (REAL)0.5, (REAL)0.5};
        int n = fm->attr_dim - 1;
        for (int i = 0; i < n; ++i) c[i % 3] = R_FMA(sh[i / 3], row[i], c[i % 3]);
        rgb[0] = R_MAX(c[0], (REAL)0);
        rgb[1] = R_MAX(c[1], (REAL)0);
        rgb[2] = R_MAX(c[2], (REAL)0);
    } else {
        rgb[0] = rgb[1] = rgb[2] = (REAL)0;
    }
}

/* cell_intersection_grad                               src/tracing/tracing_utils.cuh:91-103 */
static inline void SUF(bisector_grad)(const REAL *p, const REAL *q, const REAL *ro,
                                      const REAL *rd, REAL *g) {
    REAL fo[3], fn[3], v[3];
    for (int i = 0; i < 3; ++i) {
        fo[i] = (p[i] + q[i]) / (REAL)2;
        fn[i] = q[i] - p[i];
        v[i] = fo[i] - ro[i];
    }
    REAL num = SUF(dot3)(v, fn);
    REAL dp = SUF(dot3)(fn, rd);
    REAL den = dp * dp;
    for (int i = 0; i < 3; ++i) {
        REAL gi = R_FMA(num, rd[i], dp * (ro[i] - p[i]));
        g[i] = gi / den;
    }
}

/* One scan of the current cell's faces: nearest exit.   src/tracing/tracing_utils.cuh:27-67
 * Returns the winning face slot (absolute CSR index) or RFO_NONE; *t1 is +inf if none.
 *
 * The reference divides every face and keeps a running minimum of the rounded quotients with a strict '<'
 * (tracing_utils.cuh:43-67): the exit is the face with the smallest ROUNDED t = num/dp among those with dp > 0, the
 * lowest index among equal quotients; num = ((P + o/2) - O).o and dp = o.d in that association.  That is what
 * SUF(scan_cell_reference) evaluates, literally, and what "the scan" means everywhere in this repository.
 *
 * rfo_scan_mode 1 ("filtered") evaluates THE SAME function the way the HIP kernels do (radfoam_amd/csrc/rf_kernels.hip,
 * "the face scan"): lists padded to four entries with scaled copies, a pairwise tournament on cross-multiplied products,
 * the minimum bit distance of all compared products as a certificate, and the dividing scan for cells whose
 * certificate fails.  It exists so that the claim "filtered == reference, bit for bit" is tested on the CPU over
 * tens of millions of cell scans (tests/test_oracle.py), with the number of contested cells counted. */
static inline uint32_t SUF(scan_cell_reference)(const SUF(foam_t) *fm, uint32_t cell, const REAL *P,
                                                const REAL *ro, const REAL *rd, REAL *t1_out) {
    const uint32_t b = fm->offsets[cell], e = fm->offsets[cell + 1];
    uint32_t best = RFO_NONE;
    REAL t1q = R_INF;
    for (uint32_t f = b; f < e; ++f) {
        REAL o[3];
#if RFO_HALF_FACES
        o[0] = h2f(fm->diff[4 * (size_t)f + 0]);
        o[1] = h2f(fm->diff[4 * (size_t)f + 1]);
        o[2] = h2f(fm->diff[4 * (size_t)f + 2]);
#else
        const REAL *Q = fm->points + 3 * (size_t)fm->adj[f];
        o[0] = Q[0] - P[0];
        o[1] = Q[1] - P[1];
        o[2] = Q[2] - P[2];
#endif
        REAL v[3];
        for (int i = 0; i < 3; ++i) v[i] = (P[i] + o[i] / (REAL)2) - ro[i];
        REAL dpq = SUF(dot3)(o, rd);
        REAL tq = SUF(dot3)(v, o) / dpq;
        if (dpq > (REAL)0 && tq < t1q) {
            t1q = tq;
            best = f;
        }
    }
    *t1_out = t1q;
    return best;
}

#if RFO_HALF_FACES
/* |bits(a) - bits(b)| as unsigned integers (v_sad_u32) */
static inline uint32_t SUF(bit_distance)(float a, float b) {
    const uint32_t x = f2u(a), y = f2u(b);
    return x > y ? x - y : y - x;
}

/* offset of entry q of the cell's list PADDED to a multiple of four, as the kernels' face tables hold it: real faces as
 * they are; padding = the first entry of the block times 2^(position in the block), zero if that leaves fp16 (pad_offset,
 * rf_kernels.hip; the kernels' side of that branch runs on the scaled_2p13 / scaled_2p14 foams of
 * tests/test_gpu_foam_zoo.py) */
static inline void SUF(padded_offset)(const SUF(foam_t) *fm, uint32_t b, uint32_t cnt, uint32_t q, float *o) {
    if (q < cnt) {
        for (int i = 0; i < 3; ++i) o[i] = h2f(fm->diff[4 * (size_t)(b + q) + i]);
        return;
    }
    uint16_t h[3];
    int over = 0;
    for (int i = 0; i < 3; ++i) {
        h[i] = f2h(h2f(fm->diff[4 * (size_t)(b + (q & ~3u)) + i]) * (float)(1u << (q & 3u)));
        over |= (h[i] & 0x7C00u) == 0x7C00u;
    }
    for (int i = 0; i < 3; ++i) o[i] = over ? 0.0f : h2f(h[i]);
}

/* the kernels' dividing scan (scan_faces_strict): the reference's loop over the PADDED list.  A padding entry is a copy of
 * its block's first face further along the same normal and never wins (its quotient is never smaller, its index higher);
 * should one win all the same it stands for the face it copies, as its link in the kernels' tables does. */
static inline uint32_t SUF(scan_cell_strict_padded)(const SUF(foam_t) *fm, uint32_t cell, const float *P, const float *ro,
                                                    const float *rd, float *t1_out) {
    const uint32_t b = fm->offsets[cell], e = fm->offsets[cell + 1];
    const uint32_t cnt = e - b, padded = (cnt + 3u) & ~3u;
    uint32_t best = RFO_NONE;
    float t1q = INFINITY;
    for (uint32_t q = 0; q < padded; ++q) {
        float o[3], v[3];
        SUF(padded_offset)(fm, b, cnt, q, o);
        for (int i = 0; i < 3; ++i) v[i] = fmaf(o[i], 0.5f, P[i]) - ro[i];
        const float dpq = dot3_f32(o, rd);
        const float tq = dot3_f32(v, o) / dpq;
        if (dpq > 0.0f && tq < t1q) {
            t1q = tq;
            best = q < cnt ? q : (q & ~3u);
        }
    }
    *t1_out = t1q;
    return best != RFO_NONE ? b + best : RFO_NONE;
}

/* the kernels' evaluation; *contested: the certificate failed and the dividing scan decided */
static inline uint32_t SUF(scan_cell_filtered)(const SUF(foam_t) *fm, uint32_t cell, const float *P, const float *ro,
                                               const float *rd, float *t1_out, int *contested) {
    const uint32_t b = fm->offsets[cell], e = fm->offsets[cell + 1];
    const uint32_t cnt = e - b, padded = (cnt + 3u) & ~3u;
    float nb = INFINITY, db = 1.0f;
    uint32_t best = RFO_NONE;
    uint32_t tie = 0xFFFFFFFFu;
    for (uint32_t k = 0; k < padded; k += 2) {
        float num[2], dp[2];
        for (uint32_t j = 0; j < 2; ++j) {
            const uint32_t q = k + j;
            float o[3];
            SUF(padded_offset)(fm, b, cnt, q, o);
            float v[3];
            for (int i = 0; i < 3; ++i) v[i] = fmaf(o[i], 0.5f, P[i]) - ro[i];
            dp[j] = dot3_f32(o, rd);
            num[j] = dot3_f32(v, o);
        }
        /* products as fma(x, y, +0): a zero product is always +0 */
        const float c0 = fmaf(num[1], dp[0], 0.0f), c1 = fmaf(num[0], dp[1], 0.0f);
        const int v0 = dp[0] > 0.0f, v1 = dp[1] > 0.0f;
        const int w1 = v1 && !(v0 && !(c0 < c1));
        const float nw = w1 ? num[1] : num[0], dw = w1 ? dp[1] : dp[0];
        const float a0 = fmaf(nw, db, 0.0f), a1 = fmaf(dw, nb, 0.0f);
        if ((w1 || v0) && a0 < a1) {
            nb = nw;
            db = dw;
            best = k + (uint32_t)w1;
        }
        const uint32_t d0 = bit_distance_f32(c0, c1), d1 = bit_distance_f32(a0, a1);
        tie = d0 < tie ? d0 : tie;
        tie = d1 < tie ? d1 : tie;
    }
    float t1 = best != RFO_NONE ? nb / db : INFINITY;
    if (!(t1 < INFINITY)) best = RFO_NONE;
    /* fail-safe of the certificate's assumption (normal quotients): a zero exponent field in the winning quotient */
    const int tiny = best != RFO_NONE && (f2u(t1) & 0x7F800000u) == 0u;
    *contested = tie <= RFO_TIE_ULPS || tiny;
    if (*contested) return SUF(scan_cell_strict_padded)(fm, cell, P, ro, rd, t1_out);
    *t1_out = best != RFO_NONE ? t1 : INFINITY;
    return best != RFO_NONE ? b + best : RFO_NONE;
}
#endif

static inline uint32_t SUF(scan_cell)(const SUF(foam_t) *fm, uint32_t cell, const REAL *P,
                                      const REAL *ro, const REAL *rd, REAL *t1_out,
                                      rfo_stats *st) {
    if (st) {
        st->cells_scanned++;
        st->faces_scanned += (uint64_t)(fm->offsets[cell + 1] - fm->offsets[cell]);
    }
#if RFO_HALF_FACES
    if (rfo_scan_mode == 1) {
        int contested = 0;
        const uint32_t best = SUF(scan_cell_filtered)(fm, cell, P, ro, rd, t1_out, &contested);
        if (contested) {
#ifdef _OPENMP
#pragma omp atomic
#endif
            rfo_scan_contested++;
        }
        return best;
    }
#endif
    return SUF(scan_cell_reference)(fm, cell, P, ro, rd, t1_out);
}

/* ------------------------------------------------------------------------------------ */
/* forward, one ray                                        src/tracing/pipeline.cu:14-130 */

static uint32_t SUF(forward_ray)(const SUF(foam_t) *fm, const REAL *ray6, uint32_t start,
                                 uint32_t nq, const REAL *quantiles, REAL *rgba_out,
                                 REAL *qdepth, uint32_t *qidx, REAL *contribution,
                                 int normalize, rfo_stats *st, int atomic) {
    REAL ro[3] = {ray6[0], ray6[1], ray6[2]};
    REAL rd[3] = {ray6[3], ray6[4], ray6[5]};
    if (normalize) SUF(normalize3)(rd);
    REAL sh[16];
    SUF(sh_basis)(fm->sh_degree, rd, sh);

    REAL T = (REAL)1;
    REAL C[3] = {0, 0, 0};
    uint32_t qi = 0;
    REAL cq = (REAL)0;
    if (quantiles && nq) cq = quantiles[0];
    const REAL thr = (REAL)fm->settings.weight_threshold;

    REAL t0 = (REAL)0;
    uint32_t n = 0;
    uint32_t cur = start;
    REAL P[3] = {fm->points[3 * (size_t)cur], fm->points[3 * (size_t)cur + 1],
                 fm->points[3 * (size_t)cur + 2]};
    for (;;) {
        n++;
        if (n > fm->settings.max_intersections) break;
        REAL t1;
        uint32_t best = SUF(scan_cell)(fm, cur, P, ro, rd, &t1, st);
#if RFO_HALF_FACES
        if (rfo_path_cells && n - 1 < rfo_path_cap) {   /* rfo_trace_paths: the cells a ray scans and where it leaves them */
            rfo_path_cells[n - 1] = cur;
            rfo_path_t1[n - 1] = best == RFO_NONE ? R_INF : t1;
        }
#endif
        if (best == RFO_NONE) break;
        uint32_t nxt = fm->adj[best];
        const REAL *Q = fm->points + 3 * (size_t)nxt;
        if (st) st->hops++;
        if (t1 > t0) {
            REAL rgb[3], s;
            SUF(load_attributes)(fm, sh, cur, rgb, &s);
            if (st) {
                st->segments++;
                if (s > (REAL)1e-6f) st->segments_lit++;
            }
            REAL dt = R_MAX(t1 - t0, (REAL)0);
            REAL alpha = (REAL)1 - R_EXP(-s * dt);
            REAL w = T * alpha;
            if (contribution) SUF(acc)(contribution + cur, w, atomic);
            C[0] = R_FMA(w, rgb[0], C[0]);
            C[1] = R_FMA(w, rgb[1], C[1]);
            C[2] = R_FMA(w, rgb[2], C[2]);
            REAL Tn = T * ((REAL)1 - alpha);
            while (qi < nq && Tn < cq) {
                qdepth[qi] = t0 + R_LOG(T / cq) / s;
                qidx[qi] = cur;
                qi++;
                if (qi < nq) cq = quantiles[qi];
            }
            T = Tn;
            if (!(T > thr)) break;
        }
        t0 = R_MAX(t0, t1);
        cur = nxt;
        P[0] = Q[0];
        P[1] = Q[1];
        P[2] = Q[2];
    }
    while (qi < nq) {
        qdepth[qi] = (REAL)-1;
        qidx[qi] = RFO_NONE;
        qi++;
    }
    rgba_out[0] = C[0];
    rgba_out[1] = C[1];
    rgba_out[2] = C[2];
    rgba_out[3] = (REAL)1 - T;
    return n;
}

/* ------------------------------------------------------------------------------------ */
/* backward, one ray                                     src/tracing/pipeline.cu:132-343
 *
 * strict != 0 reproduces the reference exactly, including (SURVEY.md Appendix A.4):
 *   - the gradients accumulated for the last visited cell and its exit neighbour are never
 *     written (kernel ends right after trace(), pipeline.cu:335-343);
 *   - on the first segment prev_point is (0,0,0), so dt0/dcurrent is taken against a
 *     bisector with the world origin (pipeline.cu:212-213,294-295);
 *   - dL/dt0 gets depth_grad/s rather than depth_grad (pipeline.cu:263-265).
 * strict == 0 is the mathematically clean gradient (tails flushed, no phantom first-cell
 * term, dL/dt0 += depth_grad) used only to validate the maths against finite differences.
 * Gradients go to pg[N,3] / ag[N,A] / perr[N] with plain += (caller provides per-thread
 * or exclusive buffers).                                                                  */

static void SUF(backward_ray)(const SUF(foam_t) *fm, const REAL *ray6, uint32_t start,
                              uint32_t nq, const REAL *quantiles, const uint32_t *qidx_in,
                              const REAL *rgba, const REAL *g, const REAL *dgrad,
                              const REAL *ray_error, const SUF(sink_t) *sink, int strict) {
    const int atomic = sink->atomic && !sink->wc;
    const int want_err = sink->pe != NULL;
    REAL ro[3] = {ray6[0], ray6[1], ray6[2]};
    REAL rd[3] = {ray6[3], ray6[4], ray6[5]};
    SUF(normalize3)(rd);
    REAL sh[16];
    SUF(sh_basis)(fm->sh_degree, rd, sh);
    const int A = fm->attr_dim;
    const REAL thr = (REAL)fm->settings.weight_threshold;

    REAL err = ray_error ? *ray_error : (REAL)0;
    uint32_t qi = 0;
    REAL cq = (REAL)0;
    if (quantiles && nq) cq = quantiles[0];
    REAL cdg = (REAL)0;
    for (uint32_t i = 0; i < nq; ++i) {
        if (qidx_in[i] != RFO_NONE) {
            REAL s = fm->attributes[(size_t)qidx_in[i] * A + A - 1];
            cdg += dgrad[i] / s;
        }
    }

    REAL T = (REAL)1;
    REAL C[3] = {0, 0, 0};
    uint32_t prev = RFO_NONE;
    REAL prevP[3] = {0, 0, 0};
    REAL prev_g[3] = {0, 0, 0}, cur_g[3] = {0, 0, 0}, nxt_g[3] = {0, 0, 0};

    REAL t0 = (REAL)0;
    uint32_t n = 0;
    uint32_t cur = start;
    REAL P[3] = {fm->points[3 * (size_t)cur], fm->points[3 * (size_t)cur + 1],
                 fm->points[3 * (size_t)cur + 2]};
    uint32_t last_nxt = RFO_NONE;
    for (;;) {
        n++;
        if (n > fm->settings.max_intersections) break;
        REAL t1;
        uint32_t best = SUF(scan_cell)(fm, cur, P, ro, rd, &t1, NULL);
        if (best == RFO_NONE) break;
        uint32_t nxt = fm->adj[best];
        const REAL *Q = fm->points + 3 * (size_t)nxt;
        if (t1 > t0) {
            REAL rgb[3], s;
            SUF(load_attributes)(fm, sh, cur, rgb, &s);
            REAL dt = R_MAX(t1 - t0, (REAL)0);
            REAL alpha = (REAL)1 - R_EXP(-s * dt);
            REAL w = T * alpha;
            REAL da_ds = dt * ((REAL)1 - alpha);
            REAL da_ddt = (REAL)0;
            if (dt > (REAL)0) da_ddt = s * ((REAL)1 - alpha);

            C[0] = R_FMA(w, rgb[0], C[0]);
            C[1] = R_FMA(w, rgb[1], C[1]);
            C[2] = R_FMA(w, rgb[2], C[2]);
            if (want_err) {
                REAL *xpg, *xpe;
                (void)SUF(sink_row)(sink, cur, A, &xpg, &xpe);
                SUF(sink_add)(sink, xpe, w * err, atomic);
            }

            REAL dL_drgb[3] = {g[0] * w, g[1] * w, g[2] * w};
            REAL den = T * (((REAL)1 - alpha) + (REAL)1e-6f);
            REAL diff[3];
            for (int i = 0; i < 3; ++i) {
                REAL rest = (rgba[i] - C[i]) / den;
                diff[i] = rgb[i] - rest;
            }
            REAL dL_da = T * SUF(dot3)(diff, g);
            dL_da = dL_da + (((REAL)1 - rgba[3]) * g[3]) / (((REAL)1 - alpha) + (REAL)1e-6f);

            REAL dL_ds = dL_da * da_ds;
            REAL dL_ddt = dL_da * da_ddt;
            REAL dL_dt0 = (REAL)0;

            REAL Tn = T * ((REAL)1 - alpha);
            while (qi < nq && Tn < cq) {
                REAL gi = dgrad[qi] / s;
                dL_dt0 = dL_dt0 + (strict ? gi : dgrad[qi]);
                dL_ds = dL_ds + ((-gi) * R_LOG(T / cq)) / s;
                cdg = cdg - gi;
                qi++;
                if (qi < nq) cq = quantiles[qi];
            }
            if (qi < nq) {
                dL_ds = R_FMA(-dt, cdg, dL_ds);
                dL_ddt = R_FMA(-s, cdg, dL_ddt);
            }
            dL_dt0 = dL_dt0 + (-dL_ddt);
            REAL dL_dt1 = dL_ddt;

            REAL dt0_dprev[3] = {0, 0, 0}, dt1_dP[3], dt0_dP[3] = {0, 0, 0}, dt1_dQ[3];
            if (prev != RFO_NONE) SUF(bisector_grad)(prevP, P, ro, rd, dt0_dprev);
            SUF(bisector_grad)(P, Q, ro, rd, dt1_dP);
            if (strict || prev != RFO_NONE) SUF(bisector_grad)(P, prevP, ro, rd, dt0_dP);
            SUF(bisector_grad)(Q, P, ro, rd, dt1_dQ);

            for (int i = 0; i < 3; ++i) {
                prev_g[i] = R_FMA(dL_dt0, dt0_dprev[i], prev_g[i]);
                cur_g[i] = cur_g[i] + R_FMA(dL_dt0, dt0_dP[i], dL_dt1 * dt1_dP[i]);
                nxt_g[i] = R_FMA(dL_dt1, dt1_dQ[i], nxt_g[i]);
            }
            if (prev != RFO_NONE) {
                REAL *xpg, *xpe;
                (void)SUF(sink_row)(sink, prev, A, &xpg, &xpe);
                SUF(sink_add)(sink, xpg + 0, prev_g[0], atomic);
                SUF(sink_add)(sink, xpg + 1, prev_g[1], atomic);
                SUF(sink_add)(sink, xpg + 2, prev_g[2], atomic);
            }
            for (int i = 0; i < 3; ++i) {
                prevP[i] = P[i];
                prev_g[i] = cur_g[i];
                cur_g[i] = nxt_g[i];
                nxt_g[i] = (REAL)0;
            }
            prev = cur;
            last_nxt = nxt;
            T = Tn;

            for (int i = 0; i < 3; ++i)
                if (rgb[i] == (REAL)0) dL_drgb[i] = (REAL)0;
            REAL *xpg, *xpe;
            REAL *row = SUF(sink_row)(sink, cur, A, &xpg, &xpe);
            for (int i = 0; i < A - 1; ++i) SUF(sink_add)(sink, row + i, sh[i / 3] * dL_drgb[i % 3], atomic);
            SUF(sink_add)(sink, row + (A - 1), dL_ds, atomic);

            if (!(T > thr)) break;
        }
        t0 = R_MAX(t0, t1);
        cur = nxt;
        P[0] = Q[0];
        P[1] = Q[1];
        P[2] = Q[2];
    }
    if (!strict && prev != RFO_NONE) {
        /* clean variant: flush what the reference drops */
        REAL *apg, *bpg, *xpe;
        (void)SUF(sink_row)(sink, prev, A, &apg, &xpe);
        for (int i = 0; i < 3; ++i) SUF(sink_add)(sink, apg + i, prev_g[i], atomic);
        (void)SUF(sink_row)(sink, last_nxt, A, &bpg, &xpe);
        for (int i = 0; i < 3; ++i) SUF(sink_add)(sink, bpg + i, cur_g[i], atomic);
    }
}
