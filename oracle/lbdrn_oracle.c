/*
 * lbdrn_oracle.c -- CPU restatement of the LBDRN-MSIC per-image hot path.
 *
 * TEST INFRASTRUCTURE ONLY.  Nothing in the product (lbdrn-msic_amd/, bench.py's
 * measured leg) may link, load or call this file; only tests/, the smoke check
 * and bench.py's cpu_baseline leg use it, and only as the checker.
 *
 * Every function cites the reference lines (relative to /root/reference) it
 * restates.  The arithmetic is written out so that it is reproducible bit for
 * bit on any IEEE-754 machine: float32 everywhere the reference computes in
 * float32, each dot product a k-ordered fmaf chain that starts from the bias
 * (the order an f32 MFMA produces), sin/cos/exp as explicit polynomial
 * kernels (coefficients: oracle/derive_coeffs.py).  torch's CPU sgemm order
 * and vectorised sin are unspecified, so this file -- not torch -- defines
 * the bit pattern the HIP path has to hit; tests/test_oracle_golden.py pins
 * it to outputs of the imported reference modules within float tolerance.
 *
 * Build: gcc -O2 -fPIC -shared -ffp-contract=off -fno-fast-math (oracle/build.py)
 */
#include <math.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

/* ---------------------------------------------------------------- canonical math */

static const float TWO_OVER_PI = 0x1.45f306p-1f;
static const float PIO2_A = 0x1.921fb6p+0f, PIO2_B = -0x1.777a5cp-25f, PIO2_C = -0x1.ee59dap-50f;
static const float SIN_C0 = -0x1.555556p-3f, SIN_C1 = 0x1.11110ep-7f, SIN_C2 = -0x1.a0133p-13f,
                   SIN_C3 = 0x1.6d96dp-19f;
static const float COS_C0 = -0x1.0p-1f, COS_C1 = 0x1.555556p-5f, COS_C2 = -0x1.6c16bap-10f,
                   COS_C3 = 0x1.a0122ep-16f, COS_C4 = -0x1.245a26p-22f;
static const float LOG2E = 0x1.715476p+0f, LN2_A = 0x1.62e43p-1f, LN2_B = -0x1.05c61p-29f;
static const float EXP_C0 = 0x1.0p-1f, EXP_C1 = 0x1.5554d4p-3f, EXP_C2 = 0x1.5554ep-5f,
                   EXP_C3 = 0x1.121588p-7f, EXP_C4 = 0x1.6d4f48p-10f;

/* value of sin (quad even) or cos (quad odd) of the reduced argument, signed by quadrant */
static inline float sincos_poly(float r, int quad)
{
    float s = r * r;
    float ps = fmaf(fmaf(fmaf(SIN_C3, s, SIN_C2), s, SIN_C1), s, SIN_C0);
    float sn = fmaf(r * s, ps, r);
    float pc = fmaf(fmaf(fmaf(fmaf(COS_C4, s, COS_C3), s, COS_C2), s, COS_C1), s, COS_C0);
    float cs = fmaf(s, pc, 1.0f);
    float v = (quad & 1) ? cs : sn;
    return (quad & 2) ? -v : v;
}

/* shift 0 -> sin(x), shift 1 -> cos(x).  One branch-free path for every finite x: the
 * quadrant comes from k mod 4 in float arithmetic (exact for any integer-valued float), so no
 * float->int conversion can overflow.  Accurate to 1.5 ulp for |x| <= 2^16, to ~1e-7 absolute
 * up to 2^23; beyond that x itself is coarser than a period. NaN/Inf propagate to NaN. */
static inline float canon_sincos(float x, int shift)
{
    float k = rintf(x * TWO_OVER_PI);
    float r = fmaf(-k, PIO2_A, x);
    r = fmaf(-k, PIO2_B, r);
    r = fmaf(-k, PIO2_C, r);
    float qf = fmaf(-4.0f, floorf(k * 0.25f), k);
    int q = (qf >= 0.0f && qf < 4.0f) ? (int)qf : 0; /* NaN -> 0 */
    return sincos_poly(r, q + shift);
}

/* e^(-a), 0 <= a <= 86 */
static inline float canon_exp_neg(float a)
{
    float x = -a;
    float n = rintf(x * LOG2E);
    float r = fmaf(-n, LN2_A, x);
    r = fmaf(-n, LN2_B, r);
    float e = fmaf(fmaf(fmaf(fmaf(EXP_C4, r, EXP_C3), r, EXP_C2), r, EXP_C1), r, EXP_C0);
    float p = fmaf(r * r, e, r) + 1.0f;
    int32_t bits;
    memcpy(&bits, &p, 4);
    bits += (int32_t)n * (1 << 23);   /* (n <= 0: a multiplication, not a shift of a negative value) */
    memcpy(&p, &bits, 4);
    return p;
}

/* nn.Sigmoid: LBDRNmodel.py:75 */
static inline float canon_sigmoid(float z)
{
    float a = fabsf(z);
    a = (a > 86.0f) ? 86.0f : a; /* NaN stays NaN */
    float t = canon_exp_neg(a);
    float d = 1.0f + t;
    return (z >= 0.0f) ? 1.0f / d : t / d;
}

float orc_sin(float x) { return canon_sincos(x, 0); }
float orc_cos(float x) { return canon_sincos(x, 1); }
float orc_sigmoid(float x) { return canon_sigmoid(x); }

/* ---------------------------------------------------------------- a1: bit split */

/* LBDRNdataset.py:95-101, 131.  img [C][H][W] u16 -> msb [C][H][W] u16 (value img>>K),
 * labels [H*W][C] f32 = (img - (msb<<K)) / (2^K-1); returns max(msb) in *msb_max. */
int orc_split_bits(const uint16_t *img, int C, int H, int W, int K, uint16_t *msb, float *labels,
                   int *msb_max)
{
    if (K < 1 || K > 15) return -1;
    const float denom = (float)((1 << K) - 1);
    int mx = 0;
    const int64_t HW = (int64_t)H * W;
    for (int c = 0; c < C; ++c)
        for (int64_t n = 0; n < HW; ++n) {
            unsigned v = img[c * HW + n];
            unsigned hi = v >> K;
            unsigned lo = v - (hi << K);
            if (msb) msb[c * HW + n] = (uint16_t)hi;
            if (labels) labels[n * C + c] = (float)lo / denom;
            if ((int)hi > mx) mx = (int)hi;
        }
    if (msb_max) *msb_max = mx;
    return 0;
}

/* ---------------------------------------------------------------- a2/a3: features */

/* numpy.pad(mode='reflect') index map: LBDRNdataset.py:120-123 */
static inline int reflect_idx(int i, int n)
{
    if (n == 1) return 0;
    int period = 2 * (n - 1);
    i %= period;
    if (i < 0) i += period;
    return (i < n) ? i : period - i;
}

typedef struct {
    int C, H, W, D;
    int msb_max;     /* divisor: MSB.max(), LBDRNdataset.py:120 / decode.py:93 */
    int use_colors;  /* constants.py:11 */
    int relative;    /* constants.py:14 */
    int P;           /* positional features per axis: 0, 1 (coords) or 1+2*N_FREQ (embedding) */
    const float *rowtab; /* [H][P]  ph-derived part, LBDRNdataset.py:108-118 */
    const float *coltab; /* [W][P]  pw-derived part */
} orc_feat_cfg;

static int feat_dim(const orc_feat_cfg *g)
{
    int side = 2 * g->D + 1;
    return 2 * g->P + (g->use_colors ? g->C * side * side : 0);
}

/* one feature row for pixel (y,x): layout [rowtab | coltab | c*(side^2)+dy*side+dx] */
static void feat_row(const orc_feat_cfg *g, const uint16_t *msb, int y, int x, float *out)
{
    const int side = 2 * g->D + 1;
    const int64_t HW = (int64_t)g->H * g->W;
    /* an MSB plane that is zero everywhere is normalised by 1 (the reference divides 0 by 0 there): features 0.0f */
    const float mx = (float)(g->msb_max < 1 ? 1 : g->msb_max);
    int o = 0;
    for (int p = 0; p < g->P; ++p) out[o++] = g->rowtab[(int64_t)y * g->P + p];
    for (int p = 0; p < g->P; ++p) out[o++] = g->coltab[(int64_t)x * g->P + p];
    if (!g->use_colors) return;
    const int rel = g->relative && g->D > 0; /* LBDRNdataset.py:126 */
    for (int c = 0; c < g->C; ++c) {
        const uint16_t *pl = msb + c * HW;
        float ctr = (float)pl[(int64_t)y * g->W + x] / mx;
        for (int dy = 0; dy < side; ++dy) {
            int yy = reflect_idx(y + dy - g->D, g->H);
            for (int dx = 0; dx < side; ++dx) {
                int xx = reflect_idx(x + dx - g->D, g->W);
                float v = (float)pl[(int64_t)yy * g->W + xx] / mx;
                out[o++] = rel ? v - ctr : v;
            }
        }
    }
}

int orc_feature_dim(int C, int D, int use_colors, int P)
{
    orc_feat_cfg g = {C, 1, 1, D, 1, use_colors, 1, P, 0, 0};
    return feat_dim(&g);
}

/* LBDRNdataset.py:104-130 (dup. decode.py:77-102).  idx == NULL: rows 0..n-1 in raster order. */
int orc_features(const uint16_t *msb, int C, int H, int W, int D, int msb_max, int use_colors,
                 int relative, int P, const float *rowtab, const float *coltab,
                 const int64_t *idx, int64_t n, float *out)
{
    orc_feat_cfg g = {C, H, W, D, msb_max, use_colors, relative, P, rowtab, coltab};
    const int F = feat_dim(&g);
    for (int64_t i = 0; i < n; ++i) {
        int64_t pix = idx ? idx[i] : i;
        if (pix < 0 || pix >= (int64_t)H * W) return -2;
        feat_row(&g, msb, (int)(pix / W), (int)(pix % W), out + i * F);
    }
    return 0;
}

/* ---------------------------------------------------------------- a5: forward */

/* parameter vector in state_dict order (encode.py:124-128): for each hidden layer
 * W[bc][in] then b[bc]; last layer W[C][bc], b[C]. */
static int64_t param_count(int F, int bc, int C, int nl)
{
    int64_t n = 0;
    for (int l = 0; l < nl; ++l) n += (int64_t)bc * (l ? bc : F) + bc;
    return n + (int64_t)C * bc + C;
}
int64_t orc_param_count(int F, int bc, int C, int nl) { return param_count(F, bc, C, nl); }

/* Hidden activation of every SirenLayer of `net` (LBDRNmodel.py:37,75): 0 = Sine(w0 = 30), the default; 1 = torch.nn.ReLU(),
 * the alternative the reference names at encode.py:75 / decode.py:108.  A process-wide switch (this file is single-threaded
 * test infrastructure): oracle.py's hidden_activation() context manager sets and restores it. */
static int g_hidden_relu = 0;
void orc_set_hidden_activation(int act) { g_hidden_relu = act != 0; }

/* y[j] = b[j] then fmaf over k ascending: nn.Linear, LBDRNmodel.py:32,40 */
static void linear_row(const float *Wt, const float *b, int nout, int nin, const float *x, float *z)
{
    for (int j = 0; j < nout; ++j) {
        float acc = b[j];
        const float *w = Wt + (int64_t)j * nin;
        for (int k = 0; k < nin; ++k) acc = fmaf(x[k], w[k], acc);
        z[j] = acc;
    }
}

/* LBDRNmodel.py:79-82 for one row; zs (optional) receives the pre-activations of the hidden
 * layers [nl][bc] and hs the activations, for the backward pass. */
static void forward_row(const float *params, int F, int bc, int C, int nl, const float *x,
                        float *y, float *zs, float *hs, float *scratch)
{
    const float *p = params;
    const float *in = x;
    int nin = F;
    float *z = scratch, *h = scratch + bc;
    for (int l = 0; l < nl; ++l) {
        float *zl = zs ? zs + (int64_t)l * bc : z;
        float *hl = hs ? hs + (int64_t)l * bc : ((l & 1) ? h + bc : h);
        linear_row(p, p + (int64_t)bc * nin, bc, nin, in, zl);
        if (g_hidden_relu)
            for (int j = 0; j < bc; ++j) hl[j] = zl[j] > 0.0f ? zl[j] : 0.0f; /* nn.ReLU */
        else
            for (int j = 0; j < bc; ++j) hl[j] = canon_sincos(30.0f * zl[j], 0); /* Sine: :12-13 */
        p += (int64_t)bc * nin + bc;
        in = hl;
        nin = bc;
    }
    float zo[64];
    float *zlast = (C <= 64) ? zo : (float *)malloc(sizeof(float) * C);
    linear_row(p, p + (int64_t)C * nin, C, nin, in, zlast);
    for (int c = 0; c < C; ++c) y[c] = canon_sigmoid(zlast[c]);
    if (zlast != zo) free(zlast);
}

int orc_forward(const float *params, int F, int bc, int C, int nl, const float *x, int64_t B,
                float *y)
{
    if (nl < 1) return -1;
    float *scratch = (float *)malloc(sizeof(float) * 3 * bc);
    for (int64_t i = 0; i < B; ++i)
        forward_row(params, F, bc, C, nl, x + i * F, y + i * C, 0, 0, scratch);
    free(scratch);
    return 0;
}

/* ---------------------------------------------------------------- a11: apply + reconstruct */

/* decode.py:73-134: features from the MSB plane, forward, r = round_half_even(y*(2^K-1)),
 * out[c][y][x] = (msb<<K) + r.  y_out (optional) [H*W][C] receives the sigmoid outputs. */
int orc_decode(const uint16_t *msb, int C, int H, int W, int K, int D, int msb_max,
               int use_colors, int relative, int P, const float *rowtab, const float *coltab,
               const float *params, int bc, int nl, uint16_t *out, float *y_out)
{
    orc_feat_cfg g = {C, H, W, D, msb_max, use_colors, relative, P, rowtab, coltab};
    const int F = feat_dim(&g);
    const float scale = (float)((1 << K) - 1);
    const int64_t HW = (int64_t)H * W;
    float *x = (float *)malloc(sizeof(float) * (F + C + 3 * bc));
    float *y = x + F, *scratch = y + C;
    for (int yy = 0; yy < H; ++yy)
        for (int xx = 0; xx < W; ++xx) {
            int64_t n = (int64_t)yy * W + xx;
            feat_row(&g, msb, yy, xx, x);
            forward_row(params, F, bc, C, nl, x, y, 0, 0, scratch);
            for (int c = 0; c < C; ++c) {
                float r = rintf(y[c] * scale); /* torch.round: decode.py:131 */
                float v = (float)((unsigned)msb[c * HW + n] << K) + r; /* :134 */
                out[c * HW + n] = (uint16_t)rintf(v);
                if (y_out) y_out[n * C + c] = y[c];
            }
        }
    free(x);
    return 0;
}

/* ---------------------------------------------------------------- a9: whole-image MSE */

/* LBDRNperformance.py:18-21 over the evaluator's outputs (modified_ignite_engine.py:38-43):
 * sum over all pixels and channels of (y - label)^2, accumulated in float64; the caller
 * divides by H*W*C.  labels [H*W][C]. */
double orc_eval_sse(const uint16_t *msb, const float *labels, int C, int H, int W, int D,
                    int msb_max, int use_colors, int relative, int P, const float *rowtab,
                    const float *coltab, const float *params, int bc, int nl)
{
    orc_feat_cfg g = {C, H, W, D, msb_max, use_colors, relative, P, rowtab, coltab};
    const int F = feat_dim(&g);
    float *x = (float *)malloc(sizeof(float) * (F + C + 3 * bc));
    float *y = x + F, *scratch = y + C;
    double sse = 0.0;
    for (int yy = 0; yy < H; ++yy)
        for (int xx = 0; xx < W; ++xx) {
            int64_t n = (int64_t)yy * W + xx;
            feat_row(&g, msb, yy, xx, x);
            forward_row(params, F, bc, C, nl, x, y, 0, 0, scratch);
            for (int c = 0; c < C; ++c) {
                float d = y[c] - labels[n * C + c];
                sse += (double)(d * d);
            }
        }
    free(x);
    return sse;
}

/* ---------------------------------------------------------------- a7/a8: loss, backward, Adam */

/* One trainer update (modified_ignite_engine.py:18-27) on a given minibatch:
 * forward, LBDRNLoss (LBDRNloss.py:8-11), autograd of LBDRNmodel.py:79-82, then torch Adam
 * single-tensor math (torch/optim/adam.py: lerp_, mul_/addcmul_, addcdiv_) with defaults
 * beta=(0.9,0.999), eps=1e-8 (encode.py:84).  Gradient sums run in float64 and are rounded to
 * float32 once: the reference's sgemm order is unspecified, so this is the tolerance target
 * (1e-5 relative) of every training kernel, not a bit pattern.  The bit pattern of the generic step
 * (csrc/generic.hip) is orc_step_ordered below.  step is the 1-based Adam step count.
 * grads (optional) receives the float32 gradient vector; if apply_adam == 0 only loss/grads. */
int orc_train_step(float *params, float *m, float *v, int F, int bc, int C, int nl,
                   const float *x, const float *t, int B, double lr, int step, int apply_adam,
                   double *loss_out, float *grads)
{
    const int64_t NP = param_count(F, bc, C, nl);
    double *g = (double *)calloc(NP, sizeof(double));
    float *zs = (float *)malloc(sizeof(float) * ((int64_t)2 * nl * bc + C + 3 * bc + 2 * bc));
    float *hs = zs + (int64_t)nl * bc;
    float *y = hs + (int64_t)nl * bc;
    float *scratch = y + C;
    float *dh = scratch + 3 * bc, *dz = dh + bc;
    const float inv = 1.0f / ((float)B * (float)C);
    double loss = 0.0;
    /* per-layer parameter offsets */
    int64_t *offW = (int64_t *)malloc(sizeof(int64_t) * (nl + 1));
    int64_t o = 0;
    for (int l = 0; l < nl; ++l) { offW[l] = o; o += (int64_t)bc * (l ? bc : F) + bc; }
    offW[nl] = o;
    for (int i = 0; i < B; ++i) {
        const float *xi = x + (int64_t)i * F;
        forward_row(params, F, bc, C, nl, xi, y, zs, hs, scratch);
        /* loss and d(loss)/dz_last */
        const float *Wl = params + offW[nl];
        double *gWl = g + offW[nl], *gbl = gWl + (int64_t)C * bc;
        const float *hlast = hs + (int64_t)(nl - 1) * bc;
        for (int j = 0; j < bc; ++j) dh[j] = 0.0f;
        for (int c = 0; c < C; ++c) {
            float d = y[c] - t[(int64_t)i * C + c];
            loss += (double)(d * d);
            float dy = 2.0f * d * inv;
            float dzc = dy * (y[c] * (1.0f - y[c])); /* sigmoid backward */
            gbl[c] += dzc;
            for (int j = 0; j < bc; ++j) {
                gWl[(int64_t)c * bc + j] += (double)dzc * hlast[j];
                dh[j] = fmaf(dzc, Wl[(int64_t)c * bc + j], dh[j]);
            }
        }
        for (int l = nl - 1; l >= 0; --l) {
            const int nin = l ? bc : F;
            const float *in = l ? hs + (int64_t)(l - 1) * bc : xi;
            const float *Wc = params + offW[l];
            double *gW = g + offW[l], *gb = gW + (int64_t)bc * nin;
            const float *zl = zs + (int64_t)l * bc;
            for (int j = 0; j < bc; ++j) {
                /* d sin(30 z)/dz = cos(30 z) * 30; nn.ReLU: threshold_backward, the gradient where z > 0 */
                dz[j] = g_hidden_relu ? (zl[j] > 0.0f ? dh[j] : 0.0f)
                                      : (dh[j] * canon_sincos(30.0f * zl[j], 1)) * 30.0f;
                gb[j] += dz[j];
                for (int k = 0; k < nin; ++k) gW[(int64_t)j * nin + k] += (double)dz[j] * in[k];
            }
            if (l) {
                for (int k = 0; k < nin; ++k) {
                    float a = 0.0f;
                    for (int j = 0; j < bc; ++j) a = fmaf(dz[j], Wc[(int64_t)j * nin + k], a);
                    dh[k] = a;
                }
            }
        }
    }
    if (loss_out) *loss_out = loss / ((double)B * C);
    if (grads) for (int64_t i = 0; i < NP; ++i) grads[i] = (float)g[i];
    if (apply_adam) {
        const float b1 = 0.9f, b2 = 0.999f, eps = 1e-8f;
        const float w1 = (float)(1.0 - 0.9), w2 = (float)(1.0 - 0.999);
        const double bc1 = 1.0 - pow(0.9, step), bc2 = 1.0 - pow(0.999, step);
        const float step_size = (float)(lr / bc1);
        const float bc2s = (float)sqrt(bc2);
        (void)b1;
        for (int64_t i = 0; i < NP; ++i) {
            float gi = (float)g[i];
            m[i] = m[i] + w1 * (gi - m[i]);                 /* exp_avg.lerp_(grad, 1-beta1) */
            v[i] = v[i] * b2 + w2 * (gi * gi);              /* mul_(beta2).addcmul_(g,g,1-beta2) */
            float denom = sqrtf(v[i]) / bc2s + eps;
            params[i] = params[i] + (-step_size) * (m[i] / denom); /* addcdiv_ */
        }
    }
    free(offW);
    free(zs);
    free(g);
    return 0;
}

/* ---------------------------------------------------------------- the generic step in its own order */

/* The generic training step and autograd backward of csrc/generic.hip, restated operation by operation in scalar
 * float32 so that the result is a bit pattern (orc_train_step above stays the float64 tolerance target).  The order,
 * as generic.hip's comments state it:
 *   forward    every pre-activation a chain acc = fmaf(x[k], W[j][k], acc) from the bias, k ascending; the tape keeps
 *              cos(30 z) per hidden unit (ReLU: z > 0 ? 1 : 0)
 *   head       dz = ((2 (y - t)) * inv) * (y (1 - y)), inv = 1 / ((float)B (float)C); autograd: dz = dy * (y (1 - y))
 *   loss       float64: thread (block b, lane l) of a <<<64, 256>>> grid adds (double)(d * d) for e = 256 b + l + 16384 i,
 *              i ascending; the 256-lane tree red[l] += red[l + o], o = 128 .. 1; the 64 partials in index order
 *   GradW      the batch in slices of `slice` rows (GRAD_SLICE = 256); within a slice dW[j][k] a chain
 *              acc = fmaf(dz[b][j], in[b][k], acc) from +0, b ascending, db[j] the same chain with in = 1; the slices
 *              then added in float32, acc += part[z] from 0, z ascending
 *   BackDx     v = fmaf(dz[b][j], W[j][k], v) from 0, j ascending; Sine stores (v * cos) * 30, ReLU cos != 0 ? v : 0
 *   InputDx    the same chain, stored as it is
 *   Adam       k_adam's three lines
 * A chain that ends in a part-filled 16-wide k-tile of the MFMA GEMM runs on through fmaf(0, 0, acc), which turns an
 * accumulator of -0 into +0: pad16 restates that, so that the signs of zeros agree too.
 * `slice` and `flags` exist for tests/test_generic_step_ordered_host.py, which shows that its inputs tell these orders
 * apart; the kernels' order is slice = 256, flags = 0. */
#define ORC_REVERSE_SLICES 1 /* add the slices z descending */
#define ORC_FACTOR_RIGHT 2   /* v * (cos * 30) instead of (v * cos) * 30 */
#define ORC_DROP_LAST_ROW 4  /* the last slice loses the last row of the batch */

/* range bookkeeping: the smallest nonzero magnitude and the number of non-finite values among every product,
 * accumulator and stored value of one call (products taken exactly, in float64) */
static int g_seen_on = 0;
static double g_seen_min = 0.0;
static int64_t g_seen_bad = 0;

static inline void seen(double v)
{
    double a = fabs(v);
    if (!(a <= 1.7976931348623157e308)) ++g_seen_bad; /* Inf or NaN */
    else if (a != 0.0 && a < g_seen_min) g_seen_min = a;
}

static inline float chain(float a, float b, float acc)
{
    float r = fmaf(a, b, acc);
    if (g_seen_on) {
        seen((double)a * (double)b);
        seen(r);
    }
    return r;
}

static inline float keep(float v)
{
    if (g_seen_on) seen(v);
    return v;
}

/* a chain of n terms on 16-wide k-tiles: the zero padding of a part-filled last tile */
static inline float pad16(float acc, int64_t n) { return (n & 15) ? fmaf(0.0f, 0.0f, acc) : acc; }

static void linear_ordered(const float *Wt, const float *b, int nout, int nin, const float *x, float *z)
{
    for (int j = 0; j < nout; ++j) {
        float acc = b[j];
        const float *w = Wt + (int64_t)j * nin;
        for (int k = 0; k < nin; ++k) acc = chain(x[k], w[k], acc);
        z[j] = keep(pad16(acc, nin));
    }
}

/* gW[M][nin] and, behind it, gb[M] of one nn.Linear from dz [B][M] and its input in [B][nin] */
static void grad_ordered(const float *dz, const float *in, int B, int M, int nin, int slice, int flags,
                         float *part, float *tot, float *gW)
{
    const int N = nin + 1;
    const int64_t MN = (int64_t)M * N;
    const int nsl = (B + slice - 1) / slice;
    for (int64_t e = 0; e < MN; ++e) tot[e] = 0.0f;
    for (int zi = 0; zi < nsl; ++zi) {
        const int z = (flags & ORC_REVERSE_SLICES) ? nsl - 1 - zi : zi;
        const int b0 = z * slice;
        int b1 = b0 + slice < B ? b0 + slice : B;
        if ((flags & ORC_DROP_LAST_ROW) && z == nsl - 1) --b1;
        for (int64_t e = 0; e < MN; ++e) part[e] = 0.0f;
        for (int b = b0; b < b1; ++b) {
            const float *row_in = in + (int64_t)b * nin;
            for (int j = 0; j < M; ++j) {
                const float d = dz[(int64_t)b * M + j];
                float *p = part + (int64_t)j * N;
                for (int k = 0; k < nin; ++k) p[k] = chain(d, row_in[k], p[k]);
                p[nin] = chain(d, 1.0f, p[nin]);
            }
        }
        for (int64_t e = 0; e < MN; ++e) tot[e] = keep(tot[e] + keep(pad16(part[e], b1 - b0)));
    }
    for (int j = 0; j < M; ++j) {
        for (int k = 0; k < nin; ++k) gW[(int64_t)j * nin + k] = tot[(int64_t)j * N + k];
        gW[(int64_t)M * nin + j] = tot[(int64_t)j * N + nin];
    }
}

/* out[b][k] = sum_j dz[b][j] W[j][k], j ascending from 0: the chain of BackDx and InputDx */
static inline float back_chain(const float *dzrow, const float *W, int nup, int ncols, int k)
{
    float v = 0.0f;
    for (int j = 0; j < nup; ++j) v = chain(dzrow[j], W[(int64_t)j * ncols + k], v);
    return keep(pad16(v, nup));
}

/* One generic step (dy == NULL: lbdrn_train_step on targets t) or one generic backward from an upstream gradient
 * (dy != NULL: lbdrn_forward_tape + lbdrn_backward; t, the loss and Adam take no part).  params / m / v are updated in
 * place where apply_adam; loss_out, grads [param_count], y_out [B][C], dx_out [B][F] and range [2] (smallest nonzero
 * magnitude seen, number of non-finite values) are optional. */
int orc_step_ordered(float *params, float *m, float *v, int F, int bc, int C, int nl, const float *x,
                     const float *t, const float *dy, int B, double lr, int64_t step, int apply_adam, int slice,
                     int flags, float *loss_out, float *grads, float *y_out, float *dx_out, double *range)
{
    if (nl < 1 || B < 1 || slice < 1 || (!dy && !t)) return -1;
    if (!dy && apply_adam && (!m || !v || step < 1)) return -1;
    g_seen_on = range != 0;
    g_seen_min = 1.7976931348623157e308;
    g_seen_bad = 0;
    const int relu = g_hidden_relu;
    const int64_t NP = param_count(F, bc, C, nl);
    const int64_t act = (int64_t)B * bc, total = (int64_t)B * C;
    const int rows = bc > C ? bc : C, cols = (bc > F ? bc : F) + 1;
    float *h = (float *)malloc(sizeof(float) * (2 * nl * act + 2 * total + 2 * act + NP + 2 * (int64_t)rows * cols + bc));
    float *cs = h + nl * act, *y = cs + nl * act, *dzl = y + total;
    float *dzp[2] = {dzl + total, dzl + total + act};
    float *g = dzp[1] + act, *part = g + NP, *tot = part + (int64_t)rows * cols, *zrow = tot + (int64_t)rows * cols;
    int64_t *off = (int64_t *)malloc(sizeof(int64_t) * (nl + 1));
    int64_t o = 0;
    for (int l = 0; l < nl; ++l) { off[l] = o; o += (int64_t)bc * (l ? bc : F) + bc; }
    off[nl] = o;

    /* forward with tape */
    for (int l = 0; l < nl; ++l) {
        const int nin = l ? bc : F;
        const float *in = l ? h + (l - 1) * act : x;
        const float *W = params + off[l];
        for (int b = 0; b < B; ++b) {
            linear_ordered(W, W + (int64_t)bc * nin, bc, nin, in + (int64_t)b * nin, zrow);
            float *hb = h + l * act + (int64_t)b * bc, *cb = cs + l * act + (int64_t)b * bc;
            for (int j = 0; j < bc; ++j) {
                const float z = zrow[j];
                if (relu) {
                    hb[j] = z > 0.0f ? z : 0.0f;
                    cb[j] = z > 0.0f ? 1.0f : 0.0f;
                } else {
                    const float a = keep(30.0f * z);
                    hb[j] = keep(canon_sincos(a, 0));
                    cb[j] = keep(canon_sincos(a, 1));
                }
            }
        }
    }
    {
        const float *W = params + off[nl];
        float *zc = (float *)malloc(sizeof(float) * C);
        for (int b = 0; b < B; ++b) {
            linear_ordered(W, W + (int64_t)C * bc, C, bc, h + (nl - 1) * act + (int64_t)b * bc, zc);
            for (int c = 0; c < C; ++c) y[(int64_t)b * C + c] = keep(canon_sigmoid(zc[c]));
        }
        free(zc);
    }
    if (y_out) memcpy(y_out, y, sizeof(float) * total);

    /* head */
    if (dy) {
        for (int64_t e = 0; e < total; ++e) dzl[e] = keep(dy[e] * keep(y[e] * keep(1.0f - y[e])));
    } else {
        const float inv = 1.0f / ((float)B * (float)C);
        for (int64_t e = 0; e < total; ++e) {
            const float d = keep(y[e] - t[e]);
            const float dyv = keep(keep(2.0f * d) * inv);
            dzl[e] = keep(dyv * keep(y[e] * keep(1.0f - y[e])));
        }
        /* loss: k_loss_grad<<<64, 256>>> + k_finish_loss */
        double partial[64], red[256], s = 0.0;
        for (int blk = 0; blk < 64; ++blk) {
            for (int ln = 0; ln < 256; ++ln) {
                double acc = 0.0;
                for (int64_t e = (int64_t)blk * 256 + ln; e < total; e += 64 * 256) {
                    const float d = y[e] - t[e];
                    acc += (double)keep(d * d);
                }
                red[ln] = acc;
            }
            for (int w = 128; w > 0; w >>= 1)
                for (int ln = 0; ln < w; ++ln) red[ln] += red[ln + w];
            partial[blk] = red[0];
        }
        for (int i = 0; i < 64; ++i) s += partial[i];
        if (loss_out) *loss_out = keep((float)(s / (double)total));
    }

    /* backward */
    grad_ordered(dzl, h + (nl - 1) * act, B, C, bc, slice, flags, part, tot, g + off[nl]);
    const float *dz_up = dzl, *W_up = params + off[nl];
    int n_up = C;
    for (int l = nl - 1; l >= 0; --l) {
        float *d = dzp[l & 1];
        const float *cl = cs + l * act;
        for (int b = 0; b < B; ++b)
            for (int k = 0; k < bc; ++k) {
                const float vv = back_chain(dz_up + (int64_t)b * n_up, W_up, n_up, bc, k);
                const float c = cl[(int64_t)b * bc + k];
                float r;
                if (relu) r = c != 0.0f ? vv : 0.0f;
                else if (flags & ORC_FACTOR_RIGHT) r = vv * keep(c * 30.0f);
                else r = keep(vv * c) * 30.0f;
                d[(int64_t)b * bc + k] = keep(r);
            }
        const int nin = l ? bc : F;
        grad_ordered(d, l ? h + (l - 1) * act : x, B, bc, nin, slice, flags, part, tot, g + off[l]);
        dz_up = d;
        n_up = bc;
        W_up = params + off[l];
    }
    if (dx_out)
        for (int b = 0; b < B; ++b)
            for (int k = 0; k < F; ++k) dx_out[(int64_t)b * F + k] = back_chain(dz_up + (int64_t)b * bc, params, bc, F, k);
    if (grads) memcpy(grads, g, sizeof(float) * NP);

    /* Adam: k_adam / launch_adam */
    if (!dy && apply_adam) {
        const float b2 = 0.999f, eps = 1e-8f;
        const float w1 = (float)(1.0 - 0.9), w2 = (float)(1.0 - 0.999);
        const double bc1 = 1.0 - pow(0.9, (double)step), bc2 = 1.0 - pow(0.999, (double)step);
        const float step_size = (float)(lr / bc1);
        const float bc2s = (float)sqrt(bc2);
        for (int64_t i = 0; i < NP; ++i) {
            const float gi = g[i];
            const float mi = keep(m[i] + keep(w1 * keep(gi - m[i])));
            const float vi = keep(keep(v[i] * b2) + keep(w2 * keep(gi * gi)));
            const float denom = keep(keep(sqrtf(vi)) / bc2s) + eps;
            m[i] = mi;
            v[i] = vi;
            params[i] = keep(params[i] + keep((-step_size) * keep(mi / denom)));
        }
    }
    if (range) {
        range[0] = g_seen_min;
        range[1] = (double)g_seen_bad;
    }
    g_seen_on = 0;
    free(off);
    free(h);
    return 0;
}
