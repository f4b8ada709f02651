/*
 * ace_sfno.h - C ABI of libace_sfno.so: the MI355X-native SFNO forward step.
 *
 * This is the drop-in boundary for the hot path of ai2cm/ace (`fme`): the per-step
 * forward of the Spherical Fourier Neural Operator inside the autoregressive stepper.
 * Every entry point names the reference interface it replaces (paths relative to the
 * reference tree).  The reference is pure Python on torch; its "FFI" for this path is
 * the nn.Module call boundary, so a maintainer binds these functions with ctypes
 * (see INTEGRATION.md).
 *
 * Conventions
 *   - plain pointers and sizes only; every data pointer is a DEVICE pointer to fp32
 *     unless the name ends in _host;
 *   - `stream` is a hipStream_t passed as void* (NULL = the null stream).  Calls enqueue
 *     work and return; nothing synchronises unless documented;
 *   - return value 0 = success; on failure a negative code is returned and the thread has a
 *     message.  The library never aborts.  There is one message per thread for the whole
 *     library: after a call of any family returns non-zero, ace_last_error() and every
 *     ace_<family>_last_error() return that call's message on the same thread, until the
 *     thread's next failing call.  What a getter returns on a thread with no failure before
 *     it is not specified;
 *   - tensors are contiguous, row-major, in the reference's own shapes.
 */
#ifndef ACE_SFNO_H
#define ACE_SFNO_H

#ifdef __cplusplus
extern "C" {
#endif

#define ACE_OK 0
#define ACE_ERR_INVALID (-1)   /* bad argument / unsupported configuration (Python: ValueError) */
#define ACE_ERR_RUNTIME (-2)   /* HIP runtime failure (Python: RuntimeError) */
#define ACE_ERR_STATE (-3)     /* call sequence error, e.g. forward before all weights are set */

const char* ace_last_error(void);          /* this thread's message of its last failing call, of any family */
int ace_version(void);

/* ------------------------------------------------------------------------------------------
 * Spherical harmonic transform plans.
 * Replaces RealSHT.__init__ / InverseRealSHT.__init__ (fme/sht_fix.py:69-111, 154-192): quadrature
 * nodes/weights for `grid` in {"legendre-gauss","lobatto","equiangular"}, the orthonormal
 * Condon-Shortley Legendre table (fp64 -> fp32) and the folded longitude DFT matrices.
 * lmax/mmax <= 0 select the reference defaults (lmax = nlat, or nlat-1 for lobatto;
 * mmax = nlon/2+1).  One plan serves both directions.
 * ------------------------------------------------------------------------------------------ */
typedef struct ace_sht_plan ace_sht_plan;

int ace_sht_plan_create(int nlat, int nlon, int lmax, int mmax, const char* grid, ace_sht_plan** plan);
/* Same, with the arithmetic of the Legendre stage chosen: precision 0 = exact fp32 MFMA (ace_sht_plan_create),
 * 1 = "f16x3" (error-compensated fp16 MFMA with dynamic range tracking, fp32-class accuracy; the mode the network
 * runs in by default - DESIGN.md 3.1).  Not part of the reference API (fme/sht_fix.py has one arithmetic). */
int ace_sht_plan_create_ex(int nlat, int nlon, int lmax, int mmax, const char* grid, int precision, ace_sht_plan** plan);
void ace_sht_plan_destroy(ace_sht_plan* plan);
int ace_sht_plan_dims(const ace_sht_plan* plan, int* nlat, int* nlon, int* lmax, int* mmax);
/* Which kernel family the plan's LAST Legendre launch of each direction took (test instrumentation: parity tests assert that the
 * launch they check really ran the kernel they mean to check): 0 tile engine, 1 register-resident strip kernel, 2 equatorially
 * folded strip kernel, 3 its big form (more than 96 folded latitudes: the 0.25-degree grid); -1 = no launch yet. */
int ace_sht_plan_route(const ace_sht_plan* plan, int* forward, int* inverse);
/* The plan's polar cut (test instrumentation, read-only): dead_share = the share of the spectral scratch X[m][lat] that is neither
 * stored nor loaded, kdrop = 1 when the forward table was also packed without its wholly dead leading k16-steps (small form only).
 * A plan without a cut (fp32 plans, ACE_NO_POLAR_CUT, tables without dead rows) reports 0.0 and 0. */
int ace_sht_plan_cut(const ace_sht_plan* plan, double* dead_share, int* kdrop);

/* RealSHT.forward (fme/sht_fix.py:119-139): x (n, nlat, nlon) f32 -> coeffs (n, lmax, mmax) complex64
 * stored interleaved (re, im) as 2*n*lmax*mmax floats.  May grow plan-owned scratch (hipMalloc) on
 * the first call at a given n; not capture-safe on that first call. */
int ace_sht_forward(ace_sht_plan* plan, const float* x, float* coeffs, int n, void* stream);

/* InverseRealSHT.forward (fme/sht_fix.py:202-226): coeffs (n, lmax, mmax) complex64 -> x (n, nlat, nlon). */
int ace_sht_inverse(ace_sht_plan* plan, const float* coeffs, float* x, int n, void* stream);

/* Host-only (no GPU touched): build the fp32 tables into caller buffers for inspection.
 * which: 0 = forward Legendre*quadrature wt[m][l][k] (dense, mmax*lmax*nlat floats)
 *        1 = inverse Legendre pct[m][l][k]           (dense, mmax*lmax*nlat floats)
 *        2 = quadrature nodes cos(theta) ascending (nlat doubles), 3 = quadrature weights (nlat doubles) */
int ace_sht_tables_host(int nlat, int nlon, int lmax, int mmax, const char* grid, int which, void* out_host);

/* ------------------------------------------------------------------------------------------
 * Building blocks, exported for parity tests and micro-benchmarks.
 * ------------------------------------------------------------------------------------------ */

/* nn.Conv2d(Cin, Cout, 1) [+ activation] on (n, Cin, hw) -> (n, Cout, hw)  (sfnonet.py:229, layers.py:117-124).
 * weight (Cout, Cin) row-major, bias (Cout) or NULL.  act: 0 none, 1 GELU(erf), 2 ReLU, 3 SiLU. */
int ace_conv1x1(const float* x, const float* weight, const float* bias, float* y, int n, int cin, int cout,
                long hw, int act, void* stream);

/* Same contraction on the compensated-fp16 engine ("f16x3": both operands split hi+lo fp16, three exact-product
 * MFMAs, fp32 accumulation).  Test / micro-benchmark entry: prepares the weight planes on every call and synchronises. */
int ace_conv1x1_f16x3(const float* x, const float* weight, const float* bias, float* y, int n, int cin, int cout,
                      long hw, int act, void* stream);

/* The whole fused contract of the tile GEMM engines (every 1x1 convolution that is not on one of the packed / weight-stationary
 * kernels), one launch, on the engine the caller names:
 *
 *   y = min(act(W . affine(x || x2) + bias + (res * res_scale + res_shift)), cap) * out_scale + out_shift
 *
 *   x (n, cin, hw) and the optional second source x2 (n, cin2, hw) are contracted as ONE (cin + cin2)-channel input without a
 *   concatenated copy; weight (cout, cin + cin2) row-major, contiguous; bias (cout) or NULL;
 *   in_scale / in_shift (n, cin + cin2), both or neither: the affine applied to the inputs as they are loaded (a fused instance norm);
 *   res (n, cout, hw) or NULL, with res_scale / res_shift (n, cout), both or neither;
 *   out_scale / out_shift (cout), both or neither: the affine applied last (a fused de-normalisation);
 *   act as above, the activated value clamped from above by cap (INFINITY: no clamp);
 *   in_pitch / out_pitch >= hw: floats between two channels of x, x2, res / of y; a sample's channels follow each other at the
 *   same pitch (sample stride = channels x pitch).  The floats between hw and the pitch are neither read into a result nor written;
 *   out_absmax: NULL, or 64 words that receive the bit pattern of max |y| over the stored values (the maximum over the 64 words
 *   is the maximum; the entry zeroes them first).
 *   engine 0: exact fp32, register-staged operands - 16-byte loads when every base, pitch, hw and cin + cin2 allow them, 4-byte
 *             loads otherwise; any shape;
 *          1: exact fp32, operands brought to LDS directly (the weight is copied to a pitch of roundup(cin + cin2, 32), zero
 *             padded); takes no input affine and needs hw % 4 == 0, in_pitch % 4 == 0 and 16-byte aligned x, x2;
 *          2: f16x3 (weight split as above; the dynamic-range slots of the two sources are derived as the network's producers
 *             derive them: max |x| of a source, or the bound of its affine's output when one is given; GELU runs as the network
 *             runs it on this engine, erf to 1.1e-7); needs hw % 4 == 0, in_pitch % 4 == 0, 16-byte aligned x, x2 and, with an
 *             input affine, roundup(cin + cin2, 32) <= 1024.
 * What an engine does not take is ACE_ERR_INVALID with a message, never another engine.  route (optional) receives what ran:
 * family 0 register-staged with 4-byte loads, 1 register-staged with 16-byte loads, 2 direct to LDS, 3 f16x3; tile 0 = 64 x 256
 * outputs per workgroup, 1 = 128 x 128 (taken iff cout >= 128 and it wastes no more rows than 64-row tiles would).
 * Test / micro-benchmark entry: prepares its operands on every call and synchronises. */
typedef struct ace_gemm_route { int family, tile; } ace_gemm_route;
typedef struct ace_conv1x1_fused_desc {
    const float* x; const float* x2;
    const float* weight; const float* bias;
    const float* in_scale; const float* in_shift;
    const float* res; const float* res_scale; const float* res_shift;
    const float* out_scale; const float* out_shift;
    float* y;
    unsigned* out_absmax;
    int n, cin, cin2, cout;
    long hw, in_pitch, out_pitch;
    int act;
    float cap;
    int engine;
} ace_conv1x1_fused_desc;
int ace_conv1x1_fused(const ace_conv1x1_fused_desc* desc, ace_gemm_route* route, void* stream);

/* The longitude DFT stage of the spectral blocks - the first and the last kernel of every transform - as an operator, one launch, on
 * the engine the caller names, over an existing plan (which supplies H = nlat, W = nlon, Mm = mmax and the matrix form's tables; the
 * plan's own polar cut is not used).  The spectral side is the library's internal layout X[m][lat][b][re | im][c], element
 * ((m * H + lat) * bt + b) * 2 * c + ri * c + ch, Mm * H * bt * 2 * c floats.
 *
 *   inverse = 0:  spec_out[m] = (2 pi / W) sum_w (x[w] * in_scale + in_shift) e^(-2 pi i m w / W),  m < Mm
 *                 (2 pi * rfft(norm = "forward"): fme/fft.py:61-77 under the 2 pi of fme/sht_fix.py).
 *     x (bt, c, H, W), or - engine 1 only, c % 8 == 0 - the field as P-format fp16 planes xhi / xlo ([c / 8][H W][8] halves per sample,
 *     sxp halves between samples; value = (hi + lo) / 2^e with e from the bound in the 64-word range slot xslot, as a producer
 *     kernel writes them); x is then NULL.  in_scale / in_shift (bt, c), both or neither (a fused instance norm).
 *   inverse = 1:  y = irfft(spec, n = W, norm = "forward") + bias with the imaginary parts of m = 0 and of a stored m = W / 2
 *                 ignored and the wavenumbers from Mm on zero (fme/fft.py:78-96); spec as above, bias (c) or NULL, y (bt, c, H, W).
 *   mcut: NULL, or H ints on the device (engine 1 only - the matrix kernels do not look at it, so engine 0 with mcut is refused):
 *     at latitude lat the wavenumbers m >= mcut[lat] are NOT STORED by the forward transform (spec_out keeps what it held) and read
 *     as zeros, without a load, by the inverse one.
 *   out_absmax: NULL, or 64 words that receive the bit pattern of max |stored value| (the maximum over the 64 words is the maximum;
 *     the entry zeroes them first).  The forward transform's maximum deliberately covers the entries mcut drops: the published bound
 *     is what it is without the cut.
 *   ride_weight (forward, engine 1): NULL, or a 1x1-convolution weight (ride_o, ride_i) row-major whose packing into MFMA A
 *     fragments (order ride_order, the static power-of-two scale ride_scale, one sample, no fold) rides in the launch as extra
 *     workgroups, into ride_dst ((ride_o / 32) (ride_i / 16) 1024 halves).  ride_dst_alone, of the same size, always receives the
 *     same job from the stand-alone packing launch; when the riders did not ride (route: rode = 0) ride_dst is not written.
 *   engine 0: the matrix form (fp32 MFMA against the plan's cos / sin tables): any width, 16-byte loads of x when x is 16-byte
 *             aligned, W % 4 == 0 and W >= 8, of spec when it is 16-byte aligned and c % 4 == 0; takes no planes, no mcut, no rider;
 *          1: the two-level FFT form: W in {16, 24, 48, 360, 720, 1440} and a 16-byte aligned x (forward) / y (inverse).
 * What an engine does not take is ACE_ERR_INVALID with a message, never the other engine.  route (optional) receives what ran:
 * form 0 matrix with 4-byte loads, 1 matrix with 16-byte loads, 2 FFT; rows = channel rows per workgroup (0 for the matrix form);
 * units = workgroups in x * y of the grid; rode = 1 when the rider job rode in the launch.
 * Test / micro-benchmark entry: synchronises. */
typedef struct ace_dft_route { int form, rows, units, rode; } ace_dft_route;
typedef struct ace_dft_stage_desc {
    int inverse, engine, bt, c;
    const float* x; const void* xhi; const void* xlo; long sxp; const unsigned* xslot;
    const float* in_scale; const float* in_shift;
    float* spec_out;
    const float* spec; const float* bias; float* y;
    const int* mcut;
    unsigned* out_absmax;
    const float* ride_weight; int ride_o, ride_i, ride_order; float ride_scale; void* ride_dst; void* ride_dst_alone;
} ace_dft_stage_desc;
int ace_dft_stage(ace_sht_plan* plan, const ace_dft_stage_desc* desc, ace_dft_route* route, void* stream);

/* MLP.forward (fme/ace/models/modulus/layers.py:97-137): y = W2 act(W1 x + b1) + b2 on (n, cin, hw) -> (n, cout, hw),
 * on the packed-operand f16x3 engine (the hidden activation is produced and consumed as pre-split fp16 planes and
 * never exists in fp32).  Needs cin % 8 == 0, hid % 8 == 0, hw % 4 == 0.  Test / micro-benchmark entry: prepares the
 * weight planes on every call and synchronises. */
int ace_mlp_f16x3(const float* x, const float* w1, const float* b1, const float* w2, const float* b2, float* y, int n,
                  int cin, int hid, int cout, long hw, int act, void* stream);

/* _contract_dhconv (fme/ace/models/modulus/contractions.py:183-195): out[b,o,l,m] = sum_i coeffs[b,i,l,m] * weight[i,o,l]
 * on complex values; coeffs / out (n, c, L, Mm) complex64 interleaved, weight (c, c, L, 2).  Runs the network's own kernel
 * (compensated fp16 MFMA, filter streamed once; entries with m > l are not contracted and come out zero, as they are zero
 * in every SHT output).  Needs c % 128 == 0.  Test / micro-benchmark entry: prepares the filter planes on every call and
 * synchronises. */
int ace_dhconv_f16x3(const float* coeffs, const float* weight, float* out, int n, int c, int L, int Mm, void* stream);

/* The same kernel (csrc/dhconv_strip.hip) in every form it has, one launch, as the network launches it.  ace_dhconv_f16x3 is this
 * entry with groups = 1, storage = 0, no out_absmax and e_fill = 0.
 *   coeffs / out (n, c, L, Mm) complex64 interleaved.  Entries of coeffs with m > l are not read; entries of out with m > l are
 *     never stored by the kernel: they come back as e_fill, the value the internal output scratch holds before the launch
 *     (0 unless given; NaN is refused).
 *   groups = 1: weight (c, c, L, 2), out[b,o,l,m] = sum_i coeffs[b,i,l,m] weight[i,o,l]  (contractions.py:183-195).
 *   groups = G > 1: weight as the reference holds a grouped filter, (G, L, c / G [out], c / G [in], 2),
 *     out[b,g,o,l,m] = sum_i coeffs[b,g,i,l,m] weight[g,l,o,i]  (conditional_sfno/s2convolutions.py:119-135).
 *   storage 0: dense filter planes (c rows per output column); a grouped weight is expanded to (c, c, L, 2) with exact zeros first,
 *              and the kernel skips the zero blocks when c / G is a multiple or a divisor of 128;
 *           1: the diagonal blocks alone (c / G rows per output column); needs G > 1 and c / G in {32, 64, 128} or a multiple of 128.
 *   out_absmax: NULL, or 64 words that receive the bit pattern of max |out| over the stored values (the maximum over the 64 words
 *     is the maximum; the entry zeroes them first).
 * Needs c % 128 == 0, G dividing c, operands below 2^31 elements and max |coeffs| in [2^-89, 2^112) (or zero): outside it the
 * power-of-two scale of the coefficient planes is clamped and they do not hold the operator's precision.  Whatever the strip kernel
 * does not take is ACE_ERR_INVALID with a message that names the constraint, never another engine.  route (optional) receives what ran:
 * storage as above; kspan = input channels a workgroup contracts over (c, or max(c / G, 128) with zero-block skipping);
 * units[s - 1] = workgroups with s active 32-row strips (s = 1 .. 3); max_chunks = the largest number of row chunks of one (degree,
 * 128-column group); units_per_xcd = length of each of the 8 per-XCD work lists, padding included.
 * Test / micro-benchmark entry: prepares the planes on every call and synchronises. */
typedef struct ace_dhconv_route { int storage, kspan, units[3], max_chunks, units_per_xcd; } ace_dhconv_route;
typedef struct ace_dhconv_desc {
    const float* coeffs; const float* weight; float* out;
    unsigned* out_absmax;
    int n, c, L, Mm;
    int groups, storage;
    float e_fill;
} ace_dhconv_desc;
int ace_dhconv_strip_op(const ace_dhconv_desc* desc, ace_dhconv_route* route, void* stream);

/* nn.InstanceNorm2d(C, eps, affine) (sfnonet.py:593-601) on (n, C, hw); gamma/beta may be NULL. */
int ace_instance_norm(const float* x, const float* gamma, const float* beta, float eps, float* y, int n, int c,
                      long hw, void* stream);

/* ConditionalLayerNorm.forward restricted to noise conditioning (fme/core/models/conditional_sfno/layers.py:95-141,
 * 245-318): per-PIXEL layer norm over the c channels (biased variance, eps inside the sqrt, optional elementwise
 * gamma/beta (c)), then y = y_norm * (1 + W_scale noise) + W_bias noise with the 1x1 convolutions W_scale, W_bias
 * (c, noise_dim), noise (n, noise_dim, hw).  w_scale = w_bias = NULL: plain ChannelLayerNorm.  Any hw (16-byte accesses when hw % 4 == 0).
 * Test / building-block entry: allocates its statistics workspace and synchronises. */
int ace_conditional_layer_norm(const float* x, const float* noise, const float* gamma, const float* beta,
                               const float* w_scale, const float* w_bias, float eps, float* y, int n, int c,
                               int noise_dim, long hw, void* stream);

/* The same operator as the f16x3 NoiseConditionedSFNO runs it: ONE pass per 32-pixel tile - fp64 statistics, the two
 * conditioning convolutions on the matrix cores with error-compensated fp16 operands, apply - instead of a statistics and an
 * apply pass.  Needs c % 256 == 0 (c <= 1024), hw % 4 == 0 (c > 512: hw % 32 == 0), noise_dim <= 128; any other shape is ACE_ERR_INVALID (no fallback:
 * the network routes such shapes to the two-pass form itself).  Test / building-block entry: packs the weights, synchronises. */
int ace_conditional_layer_norm_f16x3(const float* x, const float* noise, const float* gamma, const float* beta,
                                     const float* w_scale, const float* w_bias, float eps, float* y, int n, int c,
                                     int noise_dim, long hw, void* stream);

/* ------------------------------------------------------------------------------------------
 * The network.  Replaces SphericalFourierNeuralOperatorNet.__init__/forward
 * (fme/ace/models/modulus/sfnonet.py:341-685, 713-749) as built by
 * SphericalFourierNeuralOperatorBuilder.build (fme/ace/registry/sfno.py:44-61).
 * ------------------------------------------------------------------------------------------ */
typedef struct ace_sfno ace_sfno;

typedef struct ace_sfno_config {
    int in_chans, out_chans;      /* n_in_channels, n_out_channels of ModuleConfig.build */
    int nlat, nlon;               /* dataset_info.img_shape */
    int embed_dim, num_layers;
    int scale_factor;             /* >= 1: the blocks between the first filter's inverse transform and the last one's forward transform
                                     work on the (nlat / sf) x (nlon / sf) Gauss-Legendre grid (sfnonet.py:467-515) */
    float hard_thresholding_fraction;
    int operator_type;            /* 0 = "diagonal", 1 = "dhconv" */
    int normalization_layer;      /* 0 = "none", 1 = "instance_norm", 2 = conditional layer norm (NoiseConditionedSFNO),
                                     3 = "layer_norm": nn.LayerNorm over (nlat, nlon), norm0 / norm1 weight and bias are (nlat, nlon) fields
                                     (sfnonet.py:584-592) */
    int activation_function;      /* 1 = "gelu", 2 = "relu", 3 = "silu" */
    int use_mlp;
    float mlp_ratio;
    int encoder_layers;
    int pos_embed, big_skip;
    int data_grid;                /* 0 = "legendre-gauss", 2 = "equiangular" */
    int max_batch;                /* workspace is sized for this many samples (B = samples x ensemble) */
    int precision;                /* 0 = exact fp32 MFMA everywhere (the reference's arithmetic);
                                     1 = "f16x3": 1x1 convolutions on compensated fp16 MFMA (hi/lo split of both
                                     operands, 3 exact-product MFMAs, fp32 accumulate): fp32-class accuracy */
    /* NoiseConditionedSFNO (fme/ace/registry/stochastic_sfno.py:266-397; normalization_layer == 2) */
    int noise_embed_dim;          /* channels of the conditioning noise */
    int affine_norms;             /* elementwise gamma/beta in the layer norms */
    int normalize_big_skip;       /* conditional layer norm on the big-skip input */
    int filter_num_groups;        /* groups of the spectral filter (weight (G, L, C/G, C/G, 2)); >= 1 */
    int residual_filter_factor;   /* 0 / 1: none; r > 1: the big skip's input is band-limited on the data grid to lmax = nlat / r,
                                     mmax = nlon / r / 2 + 1 (sfnonet.py:473-497, 715-716) */
} ace_sfno_config;

int ace_sfno_create(const ace_sfno_config* cfg, ace_sfno** net);
void ace_sfno_destroy(ace_sfno* net);

/* Upload one parameter by its reference state_dict name: "pos_embed", "encoder.0.weight",
 * "blocks.3.filter.filter.weight", ...  `src` is a device pointer to `numel` contiguous floats in the
 * reference's shape; the library keeps its own copy (re-laid-out where a kernel wants it), so the
 * caller may free or update `src` afterwards and must call this again after an update.
 * Synchronises `stream` before returning. */
int ace_sfno_set_weight(ace_sfno* net, const char* name, const float* src, long numel, void* stream);

/* Monotonic counter bumped by every ace_sfno_set_weight: anything a caller captured around forwards of this handle (its
 * own hipGraph of a whole rollout window) is stale once the value differs from the one seen at capture time. */
long ace_sfno_weights_generation(const ace_sfno* net);

/* SURVEY 8(b) workspace_size(handle, B): device bytes the library owns for this handle when running batches up to
 * `batch` <= max_batch - activations workspace (sized by max_batch at creation), both operand forms of the weights,
 * SHT tables.  Everything else (input, output, caller tensors) is caller-owned.  Returns -1 on a bad argument. */
long ace_sfno_workspace_size(const ace_sfno* net, int batch);

/* Number of parameters / name of parameter i / its numel, in the reference's state_dict order. */
int ace_sfno_num_weights(const ace_sfno* net);
const char* ace_sfno_weight_name(const ace_sfno* net, int i);
long ace_sfno_weight_numel(const ace_sfno* net, int i);

/* Module.__call__ (fme/core/registry/module.py:74-86): in (batch, in_chans, nlat, nlon) ->
 * out (batch, out_chans, nlat, nlon).  No allocation, no host synchronisation: capture-safe. */
int ace_sfno_forward(ace_sfno* net, const float* in, float* out, int batch, void* stream);

/* NoiseConditionedModel.forward -> conditional SphericalFourierNeuralOperatorNet.forward
 * (fme/ace/registry/stochastic_sfno.py:128-172, fme/core/models/conditional_sfno/sfnonet.py:770-824) for a net created
 * with normalization_layer == 2: `noise` is the (batch, noise_embed_dim, nlat, nlon) conditioning field on the device
 * (the host side draws it - gaussian, or isotropic through ace_sht_inverse - as the reference does).  Parameters use
 * the conditional model's state_dict names without the "conditional_model." prefix.  Same stream / allocation rules as
 * ace_sfno_forward; ace_sfno_forward itself fails for such a net. */
int ace_sfno_forward_conditioned(ace_sfno* net, const float* in, const float* noise, float* out, int batch, void* stream);
/* ... with the per-stage hipEvent timing of ace_sfno_forward_timed (synchronises). */
int ace_sfno_forward_conditioned_timed(ace_sfno* net, const float* in, const float* noise, float* out, int batch,
                                       void* stream, float* ms_per_stage, int* calls_per_stage);

/* Measurement: ace_sfno_forward with a hipEvent after every launch group on `stream` (the reference's
 * CUDATimer children, fme/core/benchmark/timer.py:105-168; block children conditional_sfno/sfnonet.py:388-437,
 * filter children s2convolutions.py:372-431).  Synchronises `stream`.  ms_host[ace_sfno_num_stages()] receives the
 * milliseconds per stage summed over blocks, calls_host (optional) the number of launch groups per stage. */
int ace_sfno_num_stages(void);
/* ace_sht_plan_route of the network's internal (legendre-gauss) plan after a forward. */
int ace_sfno_sht_route(const ace_sfno* net, int* forward, int* inverse);
/* ace_sht_plan_cut of the same plan. */
int ace_sfno_sht_cut(const ace_sfno* net, double* dead_share, int* kdrop);
/* Test instrumentation: the instance-norm affine the last forward applied.  which 0: norm0, 1: norm1, of the LAST block (all blocks
   share the tables).  scale / shift: host arrays of batch * embed_dim floats; bound: the range bound that norm published (-1 when the
   precision publishes none).  Synchronises the stream of that forward; ACE_ERR_INVALID when no instance-norm forward has run. */
int ace_sfno_norm_affine(const ace_sfno* net, int which, float* scale, float* shift, float* bound);
const char* ace_sfno_stage_name(int i);
int ace_sfno_forward_timed(ace_sfno* net, const float* in, float* out, int batch, void* stream, float* ms_host,
                           int* calls_host);

/* Debug/test tap: copy the activation after block `i` (batch, embed_dim, nlat, nlon) of the LAST
 * forward into dst.  i = -1: the encoder output (after pos_embed). Only valid with ace_sfno_set_taps(net, 1). */
int ace_sfno_set_taps(ace_sfno* net, int enable);
int ace_sfno_get_tap(ace_sfno* net, int i, float* dst, int batch, void* stream);

/* hipGraph path: captures ace_sfno_forward(in, out, batch) once per distinct (in, out, batch) and
 * replays it on `stream` afterwards (the autoregressive loop with static buffers). */
int ace_sfno_forward_graph(ace_sfno* net, const float* in, float* out, int batch, void* stream);

/* ------------------------------------------------------------------------------------------
 * Stepper glue (fme/core/packer.py:45-52 + fme/core/normalizer.py:213-236, fused).
 * srcs/dsts: DEVICE arrays of nch device pointers; strides: DEVICE array of per-sample strides (floats).
 *   pack:   dst[b][j][:] = (srcs[j][b*strides[j] + :] - mean[j]) / std[j]
 *   unpack: dsts[j][b*strides[j] + :] = src[b][j][:] * std[j] + mean[j]
 * ------------------------------------------------------------------------------------------ */
int ace_pack_normalize(const float* const* srcs, const long* strides, const float* mean, const float* std_,
                       float* dst, int batch, int nch, long hw, void* stream);
int ace_unpack_denormalize(const float* src, const float* mean, const float* std_, float* const* dsts,
                           const long* strides, int batch, int nch, long hw, void* stream);

/* ------------------------------------------------------------------------------------------
 * Global-mean removal (fme/core/step/global_mean_removal.py, applied by step_with_adjustments,
 * fme/core/step/single_module.py:650-668) folded into the stepper glue above.  Tables as there: DEVICE pointer tables, per-sample
 * strides in floats, planes of hw contiguous fp32 pixels at any 4-byte alignment.  16-byte accesses only on a (plane, sample)
 * with hw % 4 == 0 and 16-byte aligned addresses, chosen once per workgroup.  Stream-ordered; no allocation, host
 * synchronisation or atomics; no workgroup waits for another; legal inside hipGraph capture.  Errors through ace_last_error.
 *
 * K reduced planes (1 for "shared": the reference field; the processed fields for "per_channel"), named by plane_idx: DEVICE int
 * [K], indices into the nsrc entries of srcs / strides.  An index outside [0, nsrc) is not read and makes that mean NaN.
 *
 * THE REDUCTION ORDER.  C = ace_gmr_chunks(hw) chunks of 4096 pixels (the last one shorter); partials: DEVICE fp64 [batch][K][C].
 *   chunk c of plane x, pixels x[4096 c + i], i = 0 .. n - 1 (n = min(4096, hw - 4096 c)); a pixel past n counts as +0.0:
 *     a[t][q] = sum over r = 0, 1, 2, 3 in this order of (double) x[4096 c + 4 (256 r + t) + q]    t = 0 .. 255, q = 0 .. 3,
 *               starting from +0.0
 *     s[t]    = (a[t][0] + a[t][1]) + (a[t][2] + a[t][3])
 *     per group w of 64 consecutive t (lane l = t - 64 w): for off = 32, 16, 8, 4, 2, 1: s[l] = s[l] + s[l + off] for l < off
 *     partials[b][k][c] = ((s[0] + s[64]) + s[128]) + s[192]
 *   every operation an fp64 addition, rounded to nearest.  The 16-byte and the 4-byte load paths give the same bits.
 *   sample_mean[b][k] = (float) ((...((partials[b][k][0] + partials[b][k][1]) + ...) + partials[b][k][C - 1]) / (double) hw)
 *                       (chunk order; one fp64 division, one rounding to fp32) - replaces t.mean(dim=...) of
 *                       global_mean_removal.py:230 / :315, which is an fp32 sum in torch's order
 *   shift[b][k]       = clim_mean[k] - sample_mean[b][k]      fp32 subtraction (global_mean_removal.py:231 / :316)
 * Every entry below that needs a mean or a shift forms it this way from the partials: there is no other order.
 *
 *   gmr_partials:           the partials of the K planes (replaces the reduction of global_mean_removal.py:230 / :315)
 *   gmr_sample_means:       gmr_partials, then means[b][k] = sample_mean[b][k] (DEVICE fp32 [batch][K])
 *   gmr_pack_normalize:     ace_pack_normalize over nin channels with shift_idx: DEVICE int [nin], the k of channel j or -1:
 *                             k >= 0: dst[b][j][p] = ((src + shift[b][k]) - mean[j]) / std[j]   three roundings
 *                                     (global_mean_removal.py:247 / :322, then normalizer.py:221)
 *                             else:   dst[b][j][p] = (src - mean[j]) / std[j]                    as ace_pack_normalize
 *                           then nextra synthetic channels (extra_idx: DEVICE int [nextra], extra_std: DEVICE fp32 [nextra]):
 *                             dst[b][nin + e][p] = (-shift[b][extra_idx[e]]) / extra_std[e]
 *                                     (global_mean_removal.py:236-238 / :329-331; single_module.py:659)
 *                           dst is [batch][nin + nextra][hw]; shift: DEVICE fp32 [batch][K], written here (1 <= K <= nin)
 *   gmr_unpack_denormalize: ace_unpack_denormalize with shift_idx: DEVICE int [nch], the k of output channel j or -1:
 *                             k >= 0: dsts[j][...] = (src * std[j] + mean[j]) - shift[b][k]     the product rounded before the
 *                                     sum (normalizer.py:236), then one fp32 subtraction (global_mean_removal.py:265 / :347)
 *                             else:   as ace_unpack_denormalize
 *                           shift: what gmr_pack_normalize wrote.
 * ------------------------------------------------------------------------------------------ */
long ace_gmr_chunks(long hw);
int ace_gmr_partials(const float* const* srcs, const long* strides, const int* plane_idx, int nsrc, double* partials, int batch,
                     int K, long hw, void* stream);
int ace_gmr_sample_means(const float* const* srcs, const long* strides, const int* plane_idx, int nsrc, double* partials,
                         float* means, int batch, int K, long hw, void* stream);
int ace_gmr_pack_normalize(const float* const* srcs, const long* strides, const float* mean, const float* std_,
                           const int* shift_idx, const double* partials, const float* clim_mean, const int* extra_idx,
                           const float* extra_std, float* dst, float* shift, int batch, int nin, int nextra, int K, long hw,
                           void* stream);
int ace_gmr_unpack_denormalize(const float* src, const float* mean, const float* std_, float* const* dsts, const long* strides,
                               const int* shift_idx, const float* shift, int batch, int nch, int K, long hw, void* stream);

/* ------------------------------------------------------------------------------------------
 * Static spatial masking (fme/core/spatial_masking.py:98-150): data[name] = fill where round(mask) == mask_value, per plane.
 * hits: DEVICE uint8 [nmask][hw], one plane per distinct 2-D mask (broadcast over the batch), nonzero where the reference's
 * `torch.round(mask).to(torch.int64) == mask_value` holds - computed by the caller with exactly those torch ops, so the kernels
 * only select and their output is bitwise the torch path's.  mask_idx: DEVICE int [nplanes], the hit plane of plane j (-1: none);
 * fill: DEVICE fp32 [nplanes].  Pointer / stride tables as in the stepper glue above (device arrays, strides in floats).
 *   mask_planes:          dsts[j][b dst_strides[j] + p] = hit ? fill[j] : srcs[j][b src_strides[j] + p]
 *                         (srcs[j] == dsts[j]: in place; an unmasked in-place plane is skipped, an unmasked other one copied)
 *   mask_pack_normalize:  v = hit ? fill[j] : srcs[j][...]; stage[j] (stage NULL or a NULL entry: none) <- v;
 *                         j < npack: dst[b][j][p] = (v - mean[j]) / std[j] with ace_pack_normalize's roundings.  Planes
 *                         npack .. nplanes - 1 are masked and staged only.
 * float4 accesses on a (plane, sample) whose hw % 4 == 0 and whose addresses are 16-byte aligned, scalar otherwise.
 * Stream-ordered; no allocation or host synchronisation.
 * ------------------------------------------------------------------------------------------ */
const char* ace_mask_last_error(void);   /* as ace_last_error(): one message per thread for the whole library */
int ace_mask_planes(const float* const* srcs, const long* src_strides, float* const* dsts, const long* dst_strides,
                    const int* mask_idx, const unsigned char* hits, int nmask, const float* fill, int nplanes, int batch,
                    long hw, void* stream);
int ace_mask_pack_normalize(const float* const* srcs, const long* src_strides, const int* mask_idx, const unsigned char* hits,
                            int nmask, const float* fill, float* const* stage, const long* stage_strides, const float* mean,
                            const float* std_, float* dst, int npack, int nplanes, int batch, long hw, void* stream);

/* ------------------------------------------------------------------------------------------
 * The exchange of the coupled atmosphere-ocean stepper (fme/coupled/stepper.py:986-1148), ace_amd/coupled.py: two launches per
 * coupled step.  Tables are DEVICE arrays as in the stepper glue above; strides in floats; every plane has hw contiguous fp32
 * pixels at any 4-byte alignment.  16-byte accesses only on a row (plane, sample, time level) with hw % 4 == 0 and a 16-byte
 * aligned address.  Stream-ordered; no allocation, atomics or host synchronisation; argument checks on the host before the
 * first HIP call (ACE_ERR_INVALID).
 *
 * ocean_to_atmosphere: the ocean state as atmosphere forcings over T = n_inner + 1 time levels, and the prescribed initial
 * surface temperature.  Slot j has a source srcs[j] with (sample, step) strides src_strides[2j], [2j+1], a destination dsts[j]
 * with dst_strides likewise, and masks[j]: a [hw] fp32 plane or NULL; a destination value is 0 where its mask is 0
 * (tensor.where(mask != 0, 0)).  Slots:
 *   0  sea surface temperature: ocean sst -> the atmosphere's surface temperature forcing, one time level
 *   1  initial surface temperature: the atmosphere's initial condition -> the prescribed one, with m = ocean fraction of
 *      level 0 and target = slot 0's destination value:  interpolate ? m * target + (1 - m) * gen
 *                                                                    : (round-half-even(m) == 1 ? target : gen)
 *   2  ocean fraction over T levels.  ACE_COUPLE_OFRAC_CARRIED: source the atmosphere's own ocean fraction (T levels), the
 *      destination may be NULL (nothing to mask: the caller keeps its tensor).  Otherwise source the land fraction (T levels):
 *      sif0 = nan_to_num(slot 3's source) (NaN -> 0, +-inf -> +-FLT_MAX);
 *      sea_ice(t) = sif0                       ACE_COUPLE_OFRAC_FROM_SIF        (one level: slot 3's step stride is not used)
 *                 = sif0 * (1 - land(t))       ACE_COUPLE_OFRAC_FROM_OCEAN_SIF  (T levels)
 *      ocean_fraction(t) = max((1 - land(t)) - sea_ice(t), 0) with NaN kept; each a single fp32 operation, never contracted
 *   3  (predicting modes only) the ocean's sea-ice field -> sea_ice
 *   4  (predicting modes only) the same source -> its unchanged values, for an atmosphere that names sea_ice differently;
 *      destination NULL: not wanted
 *   then npass pass-through fields of one time level each (3 + npass slots when carried, 5 + npass otherwise).
 * The output is bitwise the reference's torch result where that is a number, NaN where it is NaN.
 *
 * ocean_to_atmosphere_window: the same slot tables, modes, masks, argument checks and per-value arithmetic, for a rollout whose
 * atmosphere forcings live in one static window (ace_amd/coupled_rollout.py).  The one difference: EVERY slot's destination but
 * slot 1's is a window of T = n_inner + 1 time levels with its (sample, step) strides dst_strides[2j], [2j+1] both read, and a
 * one-level product - slot 0, slot 3 under ACE_COUPLE_OFRAC_FROM_SIF, slot 4, the pass-through fields - is stored to each of
 * the T levels.  Slot 1 stays a single plane.  The value stored at a level is bitwise what ocean_to_atmosphere stores for that
 * slot; every source is still read once.  The 16-byte / scalar decision is made per row (plane, sample, level): the level rows
 * of one window may differ in alignment.  Under ACE_COUPLE_OFRAC_CARRIED slot 2's destination may be its own source (the
 * window masked in place); no other destination may overlap a source or another destination.  The same destinations may be
 * NULL as in ocean_to_atmosphere.
 *
 * atmosphere_to_ocean: for name j the mean over t of the n_inner planes srcs[j * n_inner + t] (sample stride
 * src_strides[j * n_inner + t]), summed in t order in fp64, divided by n_inner and rounded to fp32 once, stored at time level
 * slot[j] (0 or 1) of the two-level window dsts[j] ((sample, step) strides dst_strides[2j], [2j+1]); the other level is
 * filled with quiet NaN.  NaN and +-inf propagate as the sum gives them.
 * ------------------------------------------------------------------------------------------ */
#define ACE_COUPLE_MAX_NAMES 64
#define ACE_COUPLE_MAX_INNER 4096
#define ACE_COUPLE_OFRAC_CARRIED 0
#define ACE_COUPLE_OFRAC_FROM_SIF 1
#define ACE_COUPLE_OFRAC_FROM_OCEAN_SIF 2
const char* ace_couple_last_error(void);   /* as ace_last_error(): one message per thread for the whole library */
int ace_couple_ocean_to_atmosphere(const float* const* srcs, const long* src_strides, float* const* dsts,
                                   const long* dst_strides, const float* const* masks, int npass, int mode, int interpolate,
                                   int n_inner, int batch, long hw, void* stream);
int ace_couple_ocean_to_atmosphere_window(const float* const* srcs, const long* src_strides, float* const* dsts,
                                          const long* dst_strides, const float* const* masks, int npass, int mode,
                                          int interpolate, int n_inner, int batch, long hw, void* stream);
int ace_couple_atmosphere_to_ocean(const float* const* srcs, const long* src_strides, float* const* dsts,
                                   const long* dst_strides, const int* slot, int nnames, int n_inner, int batch, long hw,
                                   void* stream);

/* ------------------------------------------------------------------------------------------
 * Inference diagnostics (fme/ace/aggregator/inference: reduced.py, time_mean.py, spectrum.py), ace_amd/aggregator.py.
 * Deterministic: no float atomics, a fixed partition and combine order, fp64 accumulators; stream-ordered, no allocation
 * or host synchronisation.
 *   diag_window:   srcs: DEVICE array of nplanes pointers to (batch, steps, hw) fp32 fields; strides: DEVICE long
 *                  [nplanes][2], the sample and step strides in floats (rows of a plane contiguous).  rows: DEVICE int
 *                  [nplanes], the accumulator row of each plane; wrows: DEVICE int [nplanes], its row of weights
 *                  (DEVICE fp32 [nw][hw]; a pixel of weight 0 is skipped, NaN included).  partial: DEVICE fp64 scratch of
 *                  ace_diag_partial_doubles(nplanes, batch, steps, hw) values.  series: DEVICE fp64 [2][nrows][n_time]
 *                  += the batch mean of the per-sample weighted mean (0) and weighted std sqrt(wmean((x - wmean x)^2)) (1)
 *                  at t0 + t; NaN where a sample has no pixel of non-zero weight.  do_tsum: tsum (DEVICE fp64 [nrows][hw]) +=
 *                  acc, where acc = 0, then += x[b][t] in fp64 for every sample b (outer) and step t >= t_begin (inner): every
 *                  pixel, whatever its weight.  tsum may be NULL when do_tsum is 0.  A plane whose rows[j] or wrows[j] is out
 *                  of range contributes to nothing: no accumulator changes for it.  rows must not name one row twice (the +=
 *                  on tsum and series are not atomic); this is not checked.  The weight table and the planes may start at any
 *                  4-byte boundary.
 *   diag_spectrum: coeffs: DEVICE complex64 [nnames][planes][lmax][mmax] (the forward SHT of each plane);
 *                  spec (DEVICE fp64 [nrows][lmax]) [rows[j]][l] += sum over planes and m of |c|^2.
 *   diag_paired_window: the inference evaluator's paired metrics (fme/ace/aggregator/inference/main.py:526-732: reduced.py:221-316,
 *                  time_mean.py:246-337, zonal_mean.py:153-266 on fme/core/metrics.py:63-224) from one read of the generated and
 *                  the target planes of a window, in place of the reference's separate torch reductions per name and metric on
 *                  the fields and on their normalised copies (main.py:594-598).  gen / target: DEVICE arrays of nplanes pointers to
 *                  (batch, steps, nlat, nlon) fp32 fields with contiguous planes, and their DEVICE long [nplanes][2] sample and step
 *                  strides in floats; target[j] may be NULL: then only name j's generated-side quantities are produced.  rows,
 *                  wrows, weights (DEVICE fp32 [nw][nlat * nlon]): as diag_window; a pixel of weight 0 is skipped (NaN included),
 *                  a NaN at a non-zero weight propagates.  partial: DEVICE fp64 scratch of ace_diag_paired_partial_doubles(...)
 *                  values.  series: DEVICE fp64 [6][nrows][n_time] += at t0 + t the batch mean (samples in order) of the per-sample
 *                    0 weighted mean of gen            1 weighted std of gen sqrt(wmean((x - wmean x)^2))
 *                    2 weighted mean of target         3 weighted bias wmean(d), d = gen - target widened to fp64 first
 *                    4 weighted rmse sqrt(wmean(d^2))   5 100 (G(gen) - G(target)) / G(target), G = the weighted nan-mean of the
 *                  gradient magnitude sqrt(gy^2 + gx^2): torch.gradient with unit spacing (central differences inside, one-sided
 *                  at the first / last row and at the first / last longitude, no periodic wrap), a pixel whose gradient is NaN
 *                  leaving numerator and denominator; 2..5 only for a name with a target.  do_maps: tsum (DEVICE fp64
 *                  [2][nrows][nlat * nlon], generated then target) += the per-pixel sums over samples (outer) and steps
 *                  t >= t_begin (inner) as diag_window's, and zonal (DEVICE fp64 [2][nrows][nslots][nlat]) [side][row][slot][lat]
 *                  += (the unweighted nan-mean over longitude of row lat, NaN for an all-NaN row) / (batch * factor), for b (outer)
 *                  and t (inner) in order, at slot = (zt0 + t) / factor; slots >= nslots are dropped.  zt0: this window's first
 *                  step counted from the first step of the zonal record.  tsum and zonal may be NULL when do_maps is 0.  A plane
 *                  whose rows[j] or wrows[j] is out of range contributes to nothing.  2 <= nlat, 2 <= nlon <= 2730.  Planes and the
 *                  weight table may start at any 4-byte boundary.
 *   diag_hist_window: the evaluator's histogram metric (fme/ace/aggregator/inference/histogram.py:57-82 on
 *                  fme/core/histogram.py:74-225, n_times = 1): one dynamic histogram per (side, row), side 0 = generated, 1 =
 *                  target, both sides and all names of a window in one call.  gen / target / strides / rows: as
 *                  diag_paired_window, planes of hw contiguous fp32; target[j] may be NULL: then only the generated side of name
 *                  j is recorded.  masks: NULL, or a DEVICE array of nplanes pointers to uint8 [hw] (a NULL entry: no mask); a
 *                  pixel whose byte is non-zero is removed from both sides of plane j.  State, all DEVICE and persistent across
 *                  calls: range fp64 [2][nrows][2] = (lo, hi), a NaN lo meaning "no window yet"; counts int64
 *                  [2][nrows][n_bins]; dropped int32 [2][nrows].  scratch: 16-byte aligned DEVICE memory of the bytes
 *                  ace_diag_hist_scratch_bytes(...) returns (-1 for arguments this call would refuse).
 *                  Per (side, plane j) with v = the unmasked values of all samples and steps:
 *                    1. vmin = (double)(min v - 1e-6f), vmax = (double)(max v + 1e-6f), the epsilon added in fp32.
 *                    2. lo is NaN: lo, hi = vmin, vmax.  Otherwise, while vmin < lo: lo = hi - 2 (hi - lo), and then while
 *                       vmax > hi: hi = lo + 2 (hi - lo); each doubling replaces counts by c[i] = counts[2i] + counts[2i+1] in the
 *                       upper half (left doubling) or the lower half (right doubling) and zeros in the other half.
 *                    3. step = (hi - lo) / n_bins and bin = (lo + step) - lo in fp64 (numpy's linspace(lo, hi, n_bins + 1)[1] -
 *                       [0]).
 *                    4. every value x adds 1 to counts[idx], q = (x - (float)lo) / (float)bin in fp32 with a correctly rounded
 *                       division and no contraction, idx = n_bins - 1 where q >= n_bins, 0 where q < 0, else q truncated.
 *                  The window of a (side, plane) is dropped - lo, hi and counts unchanged, dropped[side][row] += 1 - when v holds
 *                  a non-finite value, when v is empty, or when after step 2 (float)bin is 0 or not finite or (float)lo is not
 *                  finite (a constant field whose epsilon vanishes in fp32).  The reference drops such a window too once it has
 *                  edges; on a first window it keeps the poisoned edges instead, here the next good window starts the range.
 *                  A plane whose rows[j] is out of range contributes to nothing.  rows must not name one row twice; this is not
 *                  checked.  n_bins even, 2 <= n_bins <= 1024; batch * steps <= 2^21; nplanes == 0 is a no-op.  Counts are
 *                  integers added with integer atomics: bitwise repeatable.  Three launches, no allocation, no host
 *                  synchronisation.  Planes may start at any 4-byte boundary.
 *   diag_regress_window: the evaluator's per-pixel sums over time - the regression sums of the trend and ENSO-coefficient metrics
 *                  and the near-zero counts (fme/ace/aggregator/inference/trend.py:104-147, enso/enso_coefficient.py:118-168 and
 *                  418-437, near_zero_fraction.py:147-186) - for both sides and all names of a window from one read of every
 *                  plane, in place of the reference's torch reductions per name (and, for the ENSO covariance, per sample).
 *                  gen / target / strides / rows: as diag_paired_window, planes of hw contiguous fp32 starting at any 4-byte
 *                  boundary; side 0 = generated, 1 = target; target[j] may be NULL: then only the generated side of plane j is
 *                  produced.  A plane whose rows[j] is out of range contributes to nothing.  rows must not name one row twice
 *                  (the += below are not atomic); this is not checked.  Only steps t >= t_begin enter anything (t_begin >= steps:
 *                  nothing changes); nplanes == 0 is a no-op.
 *                  Linear terms.  coef: DEVICE fp64 [nterms][batch][steps]; slot: DEVICE int [nterms][batch], the output map of
 *                  (term k, sample b) in [0, nmaps), any other value (-1) for none; maps: DEVICE fp64 [2][nrows][nmaps][hw].
 *                  For each side, plane j, map m and pixel p:  acc = 0;  for k ascending, for b ascending over the samples with
 *                  slot[k][b] == m, for t ascending from t_begin:  acc += coef[k][b][t] * (double)x[b][t][p];  then
 *                  maps[side][rows[j]][m][p] += acc.  The multiply-add is NOT contracted: the fp64 product is rounded, then
 *                  added (no fma), so a host statement in plain fp64 arithmetic reproduces it.  NaN and infinity propagate
 *                  (0 * NaN is NaN).  Every plane is read once, in (b, t) order, so the stated order holds when each map is fed
 *                  by one term; maps fed by several terms are not supported (two terms on one map interleave per (b, t); not
 *                  checked).  0 <= nmaps <= ACE_DIAG_REGRESS_MAX_MAPS = 8: a thread holds the accumulators of its pixels in
 *                  registers; more maps are refused and belong in several calls over map subsets.  nterms == 0 is allowed (maps,
 *                  coef and slot may then be NULL and no map changes); nterms <= 64.
 *                  Indicator part, on when eps is not NULL.  eps: DEVICE fp32 [nplanes]; below = x[b][t][p] <= eps[j], compared in
 *                  fp32, NaN counting as not below.  below_count: DEVICE int64 [2][nrows][hw], [side][rows[j]][p] += the number of
 *                  (b, t >= t_begin) with below, every pixel whatever its weight.  below_frac: DEVICE fp64 [2][nrows],
 *                  [side][rows[j]] += f, where f = 0, then for b ascending, t ascending from t_begin:
 *                  f += (sum over p of w[p] below) / (sum over p of w[p]), w = row wrows[j] of weights (DEVICE fp32 [nw][hw], as
 *                  diag_window); a pixel of weight 0 enters neither sum (all weights 0: NaN, the reference's 0 / 0).  Both sums
 *                  over pixels are fp64, taken per wave of 256 pixels (4 consecutive pixels per lane, then an xor butterfly), the
 *                  per-wave partials through scratch to a second stage that adds them in a fixed order: no float atomics.  A
 *                  plane whose wrows[j] is out of range takes no part in the indicator outputs (its linear terms are still
 *                  produced).  partial: DEVICE fp64 scratch of ace_diag_regress_partial_doubles(nplanes, batch, steps, hw) values
 *                  (-1 for arguments this call would refuse); needed with the indicator only.  The counts are integers, each
 *                  pixel owned by one thread: bitwise repeatable, as are the maps and fractions.  batch * steps < 2^31.
 *                  One launch, two with the indicator, however many planes; no allocation, no host synchronisation.
 *   diag_calendar_window: the evaluator's calendar metrics - the seasonal sums and the regional series behind the annual means, the
 *                  Nino 3.4 index and the tripole index (fme/ace/aggregator/inference/seasonal.py:40-69, annual.py:181-208,
 *                  enso/dynamic_index.py:65-92, ipo/ipo_index.py:43-58 and 109-131) - for both sides and all names of a window from
 *                  one read of every plane, in place of the reference's copy of every field to the host (seasonal) and its torch
 *                  reduction and .cpu() per name and region (the others).  gen / target / strides / rows: as diag_regress_window,
 *                  planes of hw contiguous fp32 starting at any 4-byte boundary; side 0 = generated, 1 = target; target[j] may be
 *                  NULL: then only the generated side of plane j is produced.  A plane whose rows[j] is out of range [0, nrows)
 *                  contributes to nothing, binned sums and series alike.  rows must not name one row twice, and no two valid
 *                  srow entries may be equal (the += and the assignments below are not atomic); this is not checked.  Only steps
 *                  t >= t_begin enter anything (t_begin >= steps: nothing changes); nplanes == 0 is a no-op.
 *                  Binned sums, on when bins is not NULL.  bin: DEVICE int [batch][steps], the bin of step (b, t) in [0, nbins),
 *                  any other value (-1) for none; bins: DEVICE fp64 [2][nrows][nbins][hw].  For each side, plane j, bin m and
 *                  pixel p:  acc = 0;  for b ascending, for t ascending from t_begin, taking only the steps with bin[b][t] == m:
 *                  acc += (double)x[b][t][p];  then bins[side][rows[j]][m][p] += acc.  A step is ADDED to its own bin and to no
 *                  other; nothing is multiplied, so a NaN or an infinity stays in the bin of its step.  (That is why the linear
 *                  terms of diag_regress_window with 0 / 1 coefficients do not serve: 0 * NaN is NaN, and one NaN step would
 *                  poison every bin, where the reference's groupby(...).sum(skipna=False) keeps it inside its season.)  A bin no
 *                  step names adds +0.  0 <= nbins <= ACE_DIAG_CALENDAR_MAX_BINS = 8: a thread holds the sums of its pixels in
 *                  registers; more bins are refused.  Each pixel is owned by one thread: bitwise repeatable.
 *                  Regional series, on when series is not NULL.  regions: DEVICE fp32 [nreg][hw]; srow: DEVICE int
 *                  [nplanes][nreg], the output row of (plane j, region r) in [0, nsrows), any other value (-1) for none; mode:
 *                  DEVICE int [nreg]; series: DEVICE fp64 [2][nsrows][batch][n_time]; weights / wrows / nw: as diag_window.  For
 *                  each (side, j, r) with a valid srow and each (b, t >= t_begin):
 *                  series[side][srow[j][r]][b][t0 + t] = num / den, an assignment, not a +=, with num = sum over p of
 *                  (double)w[p] * (double)x[b][t][p] (the product of two fp32 values is exact in fp64) and den = sum over p of
 *                  (double)w[p], over the pixels that take part:
 *                    mode 0  metrics.weighted_mean as regional_area_weighted_mean uses it (fme/core/gridded_ops.py:361-371):
 *                            w[p] = regions[r][p] * weights[wrows[j]][p], the product formed in fp32 as the reference multiplies two
 *                            fp32 tensors (gridded_ops.py:336); a pixel with w == 0 enters neither sum (NaN included), a NaN at a
 *                            pixel of non-zero weight propagates; all weights zero: NaN, the reference's 0 / 0.
 *                    mode 1  _nan_aware_regional_mean (ipo/ipo_index.py:43-58), which takes the regional weights alone:
 *                            w[p] = regions[r][p]; a pixel whose x is NaN leaves both sums, as does a pixel with w == 0; no pixel
 *                            left: NaN.
 *                  Both sums are fp64, taken per wave of 256 pixels (4 consecutive pixels per lane added in order, then an xor
 *                  butterfly), the per-wave partials through scratch to a second stage that adds them in a fixed order: no float
 *                  atomics, bitwise repeatable.  A plane whose wrows[j] is out of range takes no part in the series, in either
 *                  mode (its binned sums are still produced).  partial: DEVICE fp64 scratch of
 *                  ace_diag_calendar_partial_doubles(nplanes, nreg, batch, steps, hw) values (-1 for arguments this call would
 *                  refuse); needed with the series only.  0 <= nreg <= ACE_DIAG_CALENDAR_MAX_REGIONS = 8; t0 >= 0 and
 *                  t0 + steps <= n_time, or the call is refused.  batch * steps < 2^31.
 *                  One launch, two with the series, however many planes; no allocation, no host synchronisation.
 *   diag_ensemble_step: the evaluator's ensemble metrics at one step of a window - the almost-fair CRPS, the ensemble-mean RMSE and
 *                  the two sums behind the spread-skill ratio (fme/ace/aggregator/one_step/ensemble.py:74-173, get_crps of
 *                  fme/core/ensemble.py:4-44 with alpha = 0.95) - for all names from one read of every plane, in place of the
 *                  reference's (B, E (E - 1) / 2, H, W) tensor of member pairs and its three torch reductions per name.
 *                  gen / target / strides / rows: as diag_regress_window, planes of hw contiguous fp32 starting at any 4-byte
 *                  boundary, fields of batch = n_ic * n_members samples with sample b = i * n_members + e (member e of initial
 *                  condition i; the target is laid out the same way, member e is compared with its own target plane).  A plane
 *                  whose rows[j] is out of range [0, nrows), or whose target[j] is NULL, contributes to nothing.  rows must not
 *                  name one row twice (the += below are not atomic); this is not checked.  maps: DEVICE fp64
 *                  [nslots][4][nrows][hw]; seen: DEVICE int [nslots][nrows].
 *                  For plane j and pixel p, with g_e, y_e the fp32 values of member e of initial condition i at step t widened to
 *                  fp64, E = n_members, every sum in ascending index order and NOT contracted (products are rounded, then added:
 *                  no fma), so a host statement in plain fp64 arithmetic reproduces it:
 *                    m   = (sum_e g_e) / E
 *                    a   = (sum_e |g_e - y_e|) / E
 *                    s   = (sum_{e<f} |g_e - g_f|, e outer ascending, f inner ascending) / (E (E - 1) / 2)
 *                    c_i = a - pair_weight * s          (the host passes pair_weight = 0.5 * (1 - (1 - alpha) / 2), alpha = 0.95)
 *                    q_i = (sum_e (m - y_e)^2) / E
 *                    v_i = (sum_e (g_e - m)^2) / (E - 1)
 *                    crps = (sum_i c_i) / n_ic,   mse = (sum_i q_i) / n_ic,   var = (sum_i v_i) / n_ic
 *                    maps[slot][0][row][p] += crps;  [1] += sqrt(mse);  [2] += mse - var / E;  [3] += var
 *                  seen[slot][rows[j]] is set to 1 by any thread that meets a target value that is not NaN (a plain 4-byte store
 *                  of the constant 1, the same value from every writer); it is never cleared.  NaN and infinity propagate.
 *                  Identical members give v_i exactly 0: for fp32 g and E <= 32 the sum E * g is exact in fp64 (24 + 5 bits) and
 *                  so is its quotient by E, hence m == g and every (g_e - m)^2 is +0 - the evaluator's prescribed-cell rule tests
 *                  variance == 0.  A thread keeps the members of its pixels in registers (the target planes are streamed), so
 *                  2 <= n_members <= ACE_DIAG_ENSEMBLE_MAX_MEMBERS = 32; other counts are refused, as are t outside [0, steps),
 *                  slot outside [0, nslots) and n_ic < 1.  nplanes == 0 is a no-op.  Each pixel is owned by one thread: no
 *                  atomics, bitwise repeatable.  One launch however many planes; no allocation, no host synchronisation.
 *   diag_fill_planes: the smooth flood fill of masked fields ahead of the spectrum (fme/core/fill.py: SmoothFloodFill with its only
 *                  instantiation, num_steps = ACE_DIAG_FILL_STEPS = 4 and a 5-tap Gaussian of sigma 1; spectrum.py:331), fused with
 *                  the stacking of a spectrum chunk: dst, a contiguous DEVICE fp32 [nnames][batch][steps][nlat][nlon], is the
 *                  SHT's whole input.  srcs / strides: as diag_window, planes of nlat * nlon contiguous fp32 starting at any
 *                  4-byte boundary.  tab: DEVICE int [nnames], the mask table of name n in [0, nmasks); any other value (-1):
 *                  the planes of name n are copied unchanged, bit for bit.  Tables, built once per distinct mask on the host
 *                  (ace_amd/fill.py: fill_tables): layers DEVICE uint8 [nmasks][nlat * nlon], blurred DEVICE fp32
 *                  [nmasks][nlat * nlon].
 *                  Valid set of a mask: where it is non-zero (the rule of the weights and of ``omitted``; not the reference's
 *                  "NaN pattern of the first plane seen" - the two agree when the data is NaN exactly where the mask is zero).
 *                  A value at a masked pixel is never read into the result.
 *                  layers.  grow(S) = S and every pixel with a pixel of S in its 3 x 3 neighbourhood, longitude circular, rows
 *                  beyond the poles empty.  Simulation A: A_0 = valid, A_k = grow(A_k-1); what A_4 leaves out is the interior,
 *                  layer 5.  Simulation B: B_0 = valid and interior (the reference marks the interior valid before its expansion
 *                  loop, fill.py:267-268), B_k = grow(B_k-1); a masked pixel first in B_k has layer k (1..4), a valid pixel layer
 *                  0.  A pixel beside the interior is filled from the inside at step 1: layers taken from simulation A alone
 *                  are wrong there.  A byte above 5 marks a pixel that is never known and never filled.
 *                  blurred = blur(the 0 / 1 valid plane) computed in fp64 and rounded once to fp32, with blur(x) = the 5-tap
 *                  Gaussian g (exp(-q^2 / 2) / their sum, q = -2..2, fp64) along latitude, rows clamped to [0, nlat - 1]
 *                  (replicate), then along longitude, circular.
 *                  Per plane: x = the source at valid pixels, 0 at masked ones, then m = (sum of x over valid pixels) / (their
 *                  number) at interior pixels (computed only when the table has one).  For k = 1..4 every layer-k pixel takes (sum
 *                  of x over its 3 x 3 neighbours of layer 0, 5 or < k) / (their number), longitude circular, rows beyond the
 *                  poles not counted.  Then out = x * bv + blur(x) * (1 - bv), bv = blurred; where bv == 1 out = x and the blur
 *                  is not formed.  m, every neighbour sum, each blur pass and the blend are fp64 without contraction, in a fixed
 *                  order, and each is rounded once to fp32 (at most eight fp32 roundings on the way to a pixel; every stage is a
 *                  convex combination, so |out - the fp64 statement| <= 2^-21 max|valid x|).  A plane of a table with no valid
 *                  pixel comes out all NaN.  A non-finite value at a valid pixel propagates; how far is not specified.
 *                  scratch: DEVICE fp64 of ace_diag_fill_scratch_doubles(nnames, batch, steps, nlat, nlon) values (-1 for arguments
 *                  this call would refuse); may be NULL when nmasks is 0.  Smallest grid: nlat >= ACE_DIAG_FILL_MIN_NLAT = 2,
 *                  nlon >= ACE_DIAG_FILL_MIN_NLON = 8; nnames * batch * steps * ceil(nlat / ACE_DIAG_FILL_TILE_H) *
 *                  ceil(nlon / ACE_DIAG_FILL_TILE_W) < 2^31.  A refused call returns ACE_ERR_INVALID and writes nothing;
 *                  nnames == 0 is a no-op.  One workgroup per ACE_DIAG_FILL_TILE_H x ACE_DIAG_FILL_TILE_W tile and plane holds the
 *                  tile and a halo of 6 in LDS: one read of the source, one write of dst, no intermediate in device memory.  Two
 *                  launches (the plane means, the tiles), one when nmasks is 0; each pixel is written by one thread: no atomics,
 *                  bitwise repeatable; no allocation, no host synchronisation.
 *   diag_time_segments: the data writers' reductions over time (fme/ace/inference/data_writer/time_coarsen.py:187-196, the block
 *                  means of coarsen_factor steps; monthly.py:339-382, the sums over the steps of each calendar month), ace_amd/
 *                  data_writer.py: per-pixel sums and means over runs of consecutive steps, for all names of a window from one read
 *                  of every plane.  srcs / strides / rows: as diag_window, planes of hw contiguous fp32 starting at any 4-byte
 *                  boundary.  edges: DEVICE int [batch][nseg + 1]; segment s of sample b is the steps [lo, hi) with
 *                  lo = min(max(edges[b][s], 0), steps) and hi = min(max(edges[b][s + 1], 0), steps): every edge is clamped on
 *                  the device, so no content of this table can make the kernel read outside a plane.  hi <= lo (an edge below
 *                  its predecessor) is an empty segment; nothing asks the edges to ascend, segments cut from a table that does
 *                  not may overlap, and a step no segment covers is not read.
 *                  For plane j, sample b, segment s and pixel p:  acc = 0.0;  for t ascending from lo to hi - 1:
 *                  acc += (double)x[b][t][p];  then, both assignments, not +=:
 *                    sums  (DEVICE fp64 [nrows][batch][nseg][hw], may be NULL)  [rows[j]][b][s][p] = acc
 *                    means (DEVICE fp32 [nrows][batch][nseg][hw], may be NULL)  [rows[j]][b][s][p] = (float)(acc / (double)(hi - lo))
 *                  The adds are plain fp64 adds in step order with no reassociation and the division is the IEEE fp64 one, so a
 *                  host statement in fp64 arithmetic reproduces both outputs bit for bit.  An empty segment gives sums 0 and
 *                  means NaN (0.0 / 0.0).  NaN and infinity propagate (masked ocean fields carry NaN).  The reference means in
 *                  fp32 (torch's fp32 mean for the blocks; for the months a running fp32 update
 *                  (old_mean * old_count + new_sum) / (old_count + n) once per window); here the sum is fp64 and is rounded
 *                  once, the stance of the coupler: with u = 2^-24 and m = max |x| over the steps of one output pixel,
 *                  |means - the reference's block mean| <= (f + 2) u m for blocks of f steps.
 *                  At least one of sums and means must be given, or the call is refused (ACE_ERR_INVALID, nothing written).  A
 *                  plane whose rows[j] is out of range [0, nrows) writes nothing.  rows must not name one row twice (two
 *                  workgroups would assign the same slots); this is not checked.  nplanes == 0 or nseg == 0 is a no-op.
 *                  1 <= batch <= 65535, nplanes <= 65535 (grid dimensions), steps >= 1.  A thread keeps the sums of its four
 *                  pixels in registers and stores each segment's result as the segment closes: no scratch, each output slot
 *                  written by one thread, no atomics, bitwise repeatable.  One launch however many planes; no allocation, no
 *                  host synchronisation.
 *   diag_region_segments: the regional file writers' reduction (fme/ace/inference/data_writer/file_writer.py:505-551: a latitude /
 *                  longitude box and a selection of steps, optionally after block means over time), ace_amd/data_writer.py: the
 *                  rectangular-region counterpart of diag_time_segments, for all names of a window in one launch, written as a
 *                  compact record.  srcs / strides / rows: as diag_time_segments, planes of nlat * nlon contiguous fp32 starting
 *                  at any 4-byte boundary, sample and step strides in floats; a NULL srcs[j] or a rows[j] out of range
 *                  [0, nrows) writes nothing.  bounds: DEVICE int [batch][nseg][2]; segment s of sample b is the steps [lo, hi)
 *                  with lo = min(max(bounds[b][s][0], 0), steps) and hi = min(max(bounds[b][s][1], 0), steps): both ends are
 *                  clamped on the device, so no content of this table can make the kernel read outside a plane.  hi <= lo is an
 *                  empty segment.  Unlike edges, segments need not touch: the steps between two segments are never read, which
 *                  is what a time selection needs; segments may overlap.  The region is the rows [lat0, lat0 + nlat_r) and the
 *                  columns [lon0, lon0 + nlon_r) of the plane; there is no wrap across the date line (the reference has none,
 *                  file_writer.py:531).
 *                  For plane j, sample b, segment s and region pixel (i, k):  acc = 0.0;  for t ascending from lo to hi - 1:
 *                  acc += (double)x[b][t][lat0 + i][lon0 + k];  then, both assignments, not +=:
 *                    sums  (DEVICE fp64 [nrows][batch][nseg][nlat_r][nlon_r], may be NULL)  [rows[j]][b][s][i][k] = acc
 *                    means (DEVICE fp32 [nrows][batch][nseg][nlat_r][nlon_r], may be NULL)  [rows[j]][b][s][i][k] =
 *                                                                                          (float)(acc / (double)(hi - lo))
 *                  The adds are plain fp64 adds in step order with no reassociation or contraction and the division is the IEEE
 *                  fp64 one, so a host statement in fp64 arithmetic reproduces both outputs bit for bit.  An empty segment gives
 *                  sums 0 and means NaN (0.0 / 0.0).  NaN and infinity propagate.  A segment of one step returns the input
 *                  value, with one exception in the sign bit: 0.0 + -0.0 is +0.0, so a -0.0 input comes back as +0.0.
 *                  Nothing outside the region, or outside the steps of some segment, is read into a result; nothing outside the
 *                  nrows * batch * nseg * nlat_r * nlon_r slots of each output is written.
 *                  Refused (ACE_ERR_INVALID, a message behind ace_diag_last_error, nothing written): lat0 < 0, nlat_r < 1 or
 *                  lat0 + nlat_r > nlat, and the same for longitude; nlat < 1 or nlon < 1; neither sums nor means given; and
 *                  diag_time_segments' limits: nrows >= 1, 1 <= batch <= 65535, 0 <= nplanes <= 65535 (grid dimensions),
 *                  steps >= 1, 0 <= nseg < 2^31 - 1.  nplanes == 0 or nseg == 0 is a no-op.  rows must not name one row twice;
 *                  this is not checked.
 *                  A thread owns four consecutive pixels of the compact record and keeps their sums in registers across a
 *                  segment.  The four are one 16-byte load only when nlon_r, lon0, nlon, the base and both strides are all
 *                  multiples of 4 floats; otherwise they may lie in two region rows and are loaded one by one.  The choice is
 *                  made once per workgroup (it depends on the plane), never per load.  No scratch, each output slot written by
 *                  one thread, no atomics, bitwise repeatable.  One launch however many planes; no allocation, no host
 *                  synchronisation.
 *   diag_video_window: the evaluator's video metric (fme/ace/aggregator/inference/video.py:33-255), ace_amd/evaluator/video.py:
 *                  per time slot of the whole inference and per pixel, the means over the samples of both sides and, for the
 *                  extended videos, of their squares and of the squared error, with the smallest and largest error - for all
 *                  names and both sides of a window from one read of every plane, the accumulators staying on the device.
 *                  gen / target / strides / rows: as diag_regress_window, planes of hw contiguous fp32 starting at any 4-byte
 *                  boundary; target[j] may be NULL.  A plane whose rows[j] is out of range [0, nrows) contributes to nothing.
 *                  rows must not name one row twice (two workgroups would update the same slots); this is not checked.
 *                  mean: DEVICE fp64 [2][nrows][n_time][hw], the generated side then the target side.  sq: DEVICE fp64
 *                  [3][nrows][n_time][hw], channel 0 gen^2, 1 target^2, 2 d^2.  err: DEVICE fp32 [2][nrows][n_time][hw], min
 *                  then max.  sq and err are both NULL (the basic videos) or both given.
 *                  For plane j, step t, slot u = t0 + t and pixel p, with g_b, y_b the fp32 values of sample b:
 *                  d_b = g_b - y_b is formed in fp32, as the reference forms its error tensor; everything else is widened to
 *                  fp64; every sum runs over b ascending from 0.0 and is NOT contracted (products are rounded, then added):
 *                    sg = sum g_b   st = sum y_b   sgg = sum g_b g_b   stt = sum y_b y_b   sdd = sum (double)d_b (double)d_b
 *                    mn = min_b d_b   mx = max_b d_b
 *                  each sum is divided by (double)batch with the IEEE fp64 division, then
 *                    mean[0][row][u][p] += sg / B    mean[1][row][u][p] += st / B
 *                    sq[0][row][u][p] += sgg / B     sq[1][row][u][p] += stt / B     sq[2][row][u][p] += sdd / B
 *                    err[0][row][u][p] = min(err[0][row][u][p], mn)    err[1][row][u][p] = max(err[1][row][u][p], mx)
 *                  so a host statement in plain fp64 arithmetic reproduces the five sums bit for bit.  With assign != 0 every
 *                  one of these is a plain assignment of the window's value and the old contents are not read (the host passes
 *                  it for a window none of whose slots has been visited: up to 48 bytes per pixel and step less to read).  A
 *                  plane with a NULL target updates mean[0] and sq[0] only.  NaN and infinity propagate through the sums.  For
 *                  min and max, if any d_b is NaN or the stored value is NaN the result is NaN (payload not specified), which is
 *                  what torch.min(dim=0) and torch.minimum do; the sign of a zero result is not specified.  Every accumulator
 *                  index is formed in 64-bit (nrows * n_time * hw passes 2^31 in real use).
 *                  Refused (ACE_ERR_INVALID, a message behind ace_diag_last_error, nothing written): t0 < 0 or
 *                  t0 + steps > n_time; batch < 1 or steps < 1; steps > 65535 or nplanes > 65535 (grid dimensions; batch is a
 *                  loop and has no upper limit); mean NULL; exactly one of sq and err given.  nplanes == 0 is a no-op.
 *                  A thread owns four pixels of one (plane, step), loops over the samples with the loads of four samples of
 *                  both sides in flight ahead of the adds (which stay in sample order), and keeps its 5 fp64 sums and 2 fp32
 *                  extrema per pixel in registers: no scratch, no LDS, each slot owned by one thread, no atomics, bitwise
 *                  repeatable.  One launch however many planes; no allocation, no host synchronisation.
 * ------------------------------------------------------------------------------------------ */
const char* ace_diag_last_error(void);   /* as ace_last_error(): one message per thread for the whole library */
long ace_diag_partial_doubles(int nplanes, int batch, int steps, long hw);
int ace_diag_window(const float* const* srcs, const long* strides, const int* rows, const int* wrows, const float* weights, int nw,
                    double* partial, double* tsum, double* series, int nrows, int n_time, int t0, int t_begin, int do_tsum,
                    int nplanes, int batch, int steps, long hw, void* stream);
int ace_diag_spectrum(const void* coeffs, const int* rows, double* spec, int nrows, int nnames, long planes, int lmax, int mmax,
                      void* stream);
long ace_diag_paired_partial_doubles(int nplanes, int batch, int steps, int nlat, int nlon);
int ace_diag_paired_window(const float* const* gen, const long* gen_strides, const float* const* target, const long* target_strides,
                           const int* rows, const int* wrows, const float* weights, int nw, double* partial, double* tsum,
                           double* zonal, double* series, int nrows, int n_time, int t0, int t_begin, int do_maps, int zt0, int factor,
                           int nslots, int nplanes, int batch, int steps, int nlat, int nlon, void* stream);
long ace_diag_hist_scratch_bytes(int nplanes, int batch, int steps, long hw);
int ace_diag_hist_window(const float* const* gen, const long* gen_strides, const float* const* target, const long* target_strides,
                         const int* rows, const unsigned char* const* masks, void* scratch, double* range, long long* counts,
                         int* dropped, int nrows, int n_bins, int nplanes, int batch, int steps, long hw, void* stream);
#define ACE_DIAG_REGRESS_MAX_MAPS 8
long ace_diag_regress_partial_doubles(int nplanes, int batch, int steps, long hw);
int ace_diag_regress_window(const float* const* gen, const long* gen_strides, const float* const* target, const long* target_strides,
                            const int* rows, const double* coef, const int* slot, double* maps, const float* eps, const int* wrows,
                            const float* weights, int nw, double* partial, long long* below_count, double* below_frac, int nrows,
                            int nterms, int nmaps, int t_begin, int nplanes, int batch, int steps, long hw, void* stream);
#define ACE_DIAG_CALENDAR_MAX_BINS 8
#define ACE_DIAG_CALENDAR_MAX_REGIONS 8
long ace_diag_calendar_partial_doubles(int nplanes, int nreg, int batch, int steps, long hw);
int ace_diag_calendar_window(const float* const* gen, const long* gen_strides, const float* const* target, const long* target_strides,
                             const int* rows, const int* bin, double* bins, const float* regions, const int* srow, const int* mode,
                             const int* wrows, const float* weights, int nw, double* partial, double* series, int nrows, int nbins,
                             int nreg, int nsrows, int n_time, int t0, int t_begin, int nplanes, int batch, int steps, long hw,
                             void* stream);
#define ACE_DIAG_ENSEMBLE_MAX_MEMBERS 32
int ace_diag_ensemble_step(const float* const* gen, const long* gen_strides, const float* const* target, const long* target_strides,
                           const int* rows, double* maps, int* seen, int nrows, int slot, int nslots, double pair_weight,
                           int t, int nplanes, int n_ic, int n_members, int steps, long hw, void* stream);
#define ACE_DIAG_FILL_STEPS 4
#define ACE_DIAG_FILL_TILE_H 32
#define ACE_DIAG_FILL_TILE_W 64
#define ACE_DIAG_FILL_MIN_NLAT 2
#define ACE_DIAG_FILL_MIN_NLON 8
long ace_diag_fill_scratch_doubles(int nnames, int batch, int steps, int nlat, int nlon);
int ace_diag_fill_planes(const float* const* srcs, const long* strides, const int* tab, const unsigned char* layers,
                         const float* blurred, int nmasks, double* scratch, float* dst, int nnames, int batch, int steps, int nlat,
                         int nlon, void* stream);
int ace_diag_time_segments(const float* const* srcs, const long* strides, const int* rows, const int* edges, double* sums,
                           float* means, int nrows, int nseg, int nplanes, int batch, int steps, long hw, void* stream);
int ace_diag_region_segments(const float* const* srcs, const long* strides, const int* rows, const int* bounds, double* sums,
                             float* means, int nrows, int nseg, int nplanes, int batch, int steps, int nlat, int nlon, int lat0,
                             int nlat_r, int lon0, int nlon_r, void* stream);
int ace_diag_video_window(const float* const* gen, const long* gen_strides, const float* const* target, const long* target_strides,
                          const int* rows, double* mean, double* sq, float* err, int nrows, int n_time, int t0, int assign,
                          int nplanes, int batch, int steps, long hw, void* stream);

/* ------------------------------------------------------------------------------------------
 * Corrector step diagnostics (csrc/stepdiag.hip; fme/core/step/step_diagnostics.py and
 * fme/ace/aggregator/inference/step_diagnostics.py).  Errors are reported behind ace_diag_last_error.  All three calls are
 * stream-ordered, allocate nothing, never synchronise the host and may be captured into a graph.
 *
 * ace_stepdiag_snapshot      one launch: for k < nplanes and b < batch, dsts[k][b * dst_strides[k] + p] = srcs[k][b * src_strides[k]
 *                  + p] for p < hw.  srcs / dsts: DEVICE tables of nplanes pointers to fp32 planes at any 4-byte boundary;
 *                  src_strides / dst_strides: DEVICE int64 per-sample strides in floats.  A workgroup moves 16 bytes per access
 *                  when hw is a multiple of 4 and both bases and both strides are 16-byte aligned, 4 bytes otherwise (chosen once
 *                  per workgroup).  The engine calls it between the unpack and the in-place physics of every step.
 * ace_stepdiag_delta_window  one launch: for k < nplanes, b < batch, t < steps and p < hw, with o = outs[k] + b * out_strides[2k]
 *                  + t * out_strides[2k + 1] and s = snaps[k] + b * snap_strides[2k] + t * snap_strides[2k + 1]:
 *                  s[p] = fl32(o[p] - s[p]), one IEEE fp32 subtraction, in place over the snapshot buffer (what torch's
 *                  corrected - output gives, bit for bit).  Needs batch * steps <= 65535 (a grid dimension).
 * ace_diag_correction_window  the correction metrics of a window of deltas, two launches (the window pass and its combine).
 *                  deltas: DEVICE table of nplanes pointers to (batch, steps, hw) fp32 deltas, planes of hw contiguous floats at
 *                  any 4-byte boundary; strides: DEVICE int64 [nplanes][2] (sample, step) in floats; stds: DEVICE fp32 [nplanes];
 *                  rows / wrows / weights / nw: as ace_diag_window (weights DEVICE fp32 [nw][hw]); rows must not name one row
 *                  twice (not checked).  partial: DEVICE fp64 scratch of ace_diag_correction_partial_doubles(nplanes, batch,
 *                  steps, hw) values.  signed_sum, magnitude_sum: DEVICE fp64 [nrows][hw]; series: DEVICE fp64 [2][nrows][n_time].
 *                  Per element n = fl32(d / std_j), the correctly rounded fp32 quotient (what torch's delta / std gives),
 *                  widened to fp64 for everything that follows.  With w the weight row wrows[j] and, for a sample b and step t,
 *                  wmean(x) = sum_p w x / sum_p w over the pixels of non-zero weight:
 *                    series[0][row][t0 + t] += (1 / batch) sum_b wmean(|n|)
 *                    series[1][row][t0 + t] += (1 / batch) sum_b sqrt(wmean((n - wmean(n))^2))
 *                  samples in order.  A pixel of weight 0 is skipped, NaN included; a NaN at non-zero weight propagates; a sample
 *                  with no weighted pixel gives NaN.  Each wave reduces its 256 pixels in two passes over registers (mean, then
 *                  the central moment), the waves' partials are merged by Chan's update in a fixed order (lane strides over the
 *                  partials, then an xor butterfly), so the series agree with a plain fp64 statement to rounding (1e-12), not bit
 *                  for bit.  And at every pixel p, whatever its weight (a NaN stays a NaN, as in the reference's maps):
 *                    signed_sum[row][p] += acc_n       magnitude_sum[row][p] += acc_a
 *                  where acc_n, acc_a start at 0.0 and take n, |n| of (b, t) with b outer and t inner: a host statement in plain
 *                  fp64 reproduces them bit for bit.  A plane whose rows[j] is outside [0, nrows) or whose wrows[j] is outside
 *                  [0, nw) contributes to nothing.  One read of the delta planes; no normalised or absolute copy; no atomics, no
 *                  workgroup waits for another, bitwise repeatable.
 *                  Refused (ACE_ERR_INVALID, nothing written): nplanes or steps > 65535, batch, hw, nw or nrows < 1, t0 < 0 or
 *                  t0 + steps > n_time, a NULL argument.  nplanes == 0 is a no-op.
 * ------------------------------------------------------------------------------------------ */
int ace_stepdiag_snapshot(const float* const* srcs, const long* src_strides, float* const* dsts, const long* dst_strides, int nplanes,
                          int batch, long hw, void* stream);
int ace_stepdiag_delta_window(const float* const* outs, const long* out_strides, float* const* snaps, const long* snap_strides,
                              int nplanes, int batch, int steps, long hw, void* stream);
long ace_diag_correction_partial_doubles(int nplanes, int batch, int steps, long hw);
int ace_diag_correction_window(const float* const* deltas, const long* strides, const float* stds, const int* rows, const int* wrows,
                               const float* weights, int nw, double* partial, double* signed_sum, double* magnitude_sum,
                               double* series, int nrows, int n_time, int t0, int nplanes, int batch, int steps, long hw,
                               void* stream);

/* ------------------------------------------------------------------------------------------
 * Post-step physics (fme/core/step/single_module.py:669-716): the AtmosphereCorrector
 * (fme/core/corrector/atmosphere.py:349-398 order, 404-700 corrections), the prescribed-SST Ocean
 * (fme/core/ocean.py:167-222, fme/core/prescriber.py:54-117) and the prescribed prognostics, applied in place on the
 * denormalised output planes of one step, in the reference's order.  Four kernel launches per step (the corrections are
 * a chain of area-weighted global means), deterministic fp64 reductions, no allocation, no host synchronisation:
 * capture-safe.  A plane is a (batch, nlat, nlon) fp32 field: device pointer + per-sample stride in floats; p = NULL
 * means "absent".
 * ------------------------------------------------------------------------------------------ */
#define ACE_PHYS_MAX_LEVELS 16
#define ACE_PHYS_MAX_POSITIVE 32
#define ACE_PHYS_MAX_PRESCRIBED 8

typedef struct ace_phys_config {
    int nlat, nlon;
    int nlev;                          /* vertical layers (ak / bk have nlev + 1 entries) */
    double timestep_seconds;
    int conserve_dry_air;              /* AtmosphereCorrectorConfig.conserve_dry_air */
    int zero_global_mean_moisture_advection;
    int moisture_budget;               /* 0 none, 1 "precipitation", 2 "evaporation", 3 "advection_and_precipitation",
                                          4 "advection_and_evaporation" */
    int clip_frozen_precipitation;
    int energy_budget;                 /* 0 none, 1 "constant_temperature" */
    double unaccounted_heating;        /* EnergyBudgetConfig.constant_unaccounted_heating */
    int ocean;                         /* 0 none, 1 prescribed SST where round(ocean fraction) == 1, 2 interpolate */
    int max_batch;
} ace_phys_config;

typedef struct ace_phys_plane { float* p; long stride; } ace_phys_plane;

typedef struct ace_phys_fields {
    /* output of the step (denormalised), corrected in place; names: fme/core/atmosphere_data.py:18-43 */
    ace_phys_plane ps;                             /* surface_pressure */
    ace_phys_plane wat[ACE_PHYS_MAX_LEVELS];       /* specific_total_water_k */
    ace_phys_plane T[ACE_PHYS_MAX_LEVELS];         /* air_temperature_k */
    ace_phys_plane adv;                            /* tendency_of_total_water_path_due_to_advection */
    ace_phys_plane precip, lhf, shf;               /* precipitation_rate, latent / sensible heat flux */
    ace_phys_plane dswsfc, uswsfc, dlwsfc, ulwsfc, ulwtoa, uswtoa;
    ace_phys_plane frozen;                         /* total_frozen_precipitation_rate, or ... */
    ace_phys_plane frozen_parts[3];                /* ... ICEsfc, GRAUPELsfc, SNOWsfc (summed); all absent: zero */
    ace_phys_plane positive[ACE_PHYS_MAX_POSITIVE];   /* force_positive_names */
    int npositive;
    /* input of the step */
    ace_phys_plane ps_in;
    ace_phys_plane wat_in[ACE_PHYS_MAX_LEVELS];
    ace_phys_plane T_in[ACE_PHYS_MAX_LEVELS];
    ace_phys_plane hgt_in;                         /* surface height (or geopotential) of the input */
    /* next step's forcing / target data */
    ace_phys_plane hgt_next, dswtoa_next;
    float hgt_in_scale, hgt_next_scale;   /* 1, or 1 / 9.80616 when the field is the surface geopotential (PHIS) */
    ace_phys_plane sst, sst_target, ocean_fraction;   /* output SST, next-step SST, next-step ocean fraction */
    ace_phys_plane prescribed_dst[ACE_PHYS_MAX_PRESCRIBED], prescribed_src[ACE_PHYS_MAX_PRESCRIBED];
    int nprescribed;
} ace_phys_fields;

typedef struct ace_physics ace_physics;
const char* ace_physics_last_error(void);   /* as ace_last_error(): one message per thread for the whole library */
/* area_weights_lat_host: nlat fp32 weights of one grid column (fme/core/metrics.py:14-32, longitudinally uniform);
 * ak_host / bk_host: nlev + 1 fp32 hybrid-sigma interface coefficients (fme/core/coordinates.py:150-280).  Either may be
 * NULL when no configured correction needs it. */
int ace_physics_create(const ace_phys_config* cfg, const float* area_weights_lat_host, const float* ak_host,
                       const float* bk_host, ace_physics** out);
void ace_physics_destroy(ace_physics* phys);
/* A new initial condition: the next ace_physics_apply seeds the dry-air reference mass from its input again
 * (CorrectorState, fme/core/corrector/state.py).  Stream ordered. */
int ace_physics_reset(ace_physics* phys, void* stream);
/* Carry the reference mass across windows: (batch) fp64 on the device.  Both synchronise `stream`. */
int ace_physics_set_reference(ace_physics* phys, const double* ref_dev, int batch, void* stream);
int ace_physics_get_reference(ace_physics* phys, double* ref_dev, int* have_host, int batch, void* stream);
/* One step.  `fields` is a HOST struct of device planes (copied into the kernel arguments). */
int ace_physics_apply(ace_physics* phys, const ace_phys_fields* fields, int batch, void* stream);

/* ------------------------------------------------------------------------------------------
 * HEALPix variant (BASELINE configs[4]): the operators of the reference's HEALPix UNet (fme/ace/models/healpix/) on
 * the 12-face mesh.  Activations of one UNet level are [image = item * 12 + face][channel][row][pitch] fp32 with a row
 * pitch >= the face width, a multiple of 4 (the pitch of that level's padded faces, so that a shifted view of a padded
 * tensor is a plain GEMM operand); gap columns [width, pitch) hold defined values (zeros or finite results).  Every tensor
 * has a "bound slot": 64 unsigned words whose maximum is the bit pattern of a bound on max|x| - zeroed by the caller,
 * written by the producing call, read by the consuming convolution (compensated-fp16 arithmetic, fp32 accumulation: the
 * same fp32-class mode as the SFNO path).  No allocation or host synchronisation outside ace_hpx_weight_create.
 * ------------------------------------------------------------------------------------------ */
#define ACE_HPX_SLACK_FLOATS 16   /* floats a caller keeps allocated behind a padded tensor (zeroed by ace_hpx_pad) */
const char* ace_hpx_last_error(void);   /* as ace_last_error(): one message per thread for the whole library */
/* HEALPixPadding (healpix_paddings.py:239-611, Karlbauer et al.; "earth2grid" gives the same result): for every cell of
 * the padded mesh [12][nside + 2p][nside + 2p] the two source cells of the unpadded mesh, packed face << 24 | row << 12 |
 * column; padded = 0.5 a + 0.5 b (b == a: plain copy).  Host only. */
int ace_hpx_pad_table_host(int nside, int p, int* idx_a_host, int* idx_b_host);
/* y[item * 12 + face][c0 + ch][m][y_pitch] (m = nside + 2p rows and valid columns, gap columns zero) from
 * x[image][ch][row][x_pitch] by the table (device copies of idx_a / idx_b).  Two calls with different c0 concatenate two
 * sources along the channels (decoder skip connections); the call that writes the last channels also zeroes
 * ACE_HPX_SLACK_FLOATS behind the tensor.  amax (optional): bound slot of y (accumulates over the calls). */
int ace_hpx_pad(const float* x, long x_img_stride, long x_chan_stride, int x_pitch, float* y, int y_chans, int c0, int c,
                const int* idx_a_dev, const int* idx_b_dev, int items, int nside, int p, int y_pitch, unsigned* amax, void* stream);
/* bound slot of a tensor no ace_hpx_* call produced (the network input): amax[64] (zeroed by the caller) <- bits(max|x|). */
int ace_hpx_absmax(const float* x, long n, unsigned* amax, void* stream);
/* A convolution weight prepared for the compensated-fp16 engine: [rows][cols] row-major fp32 on the device ->
 * fp16 hi / lo planes under a power-of-two scale.  Synchronises the stream (once per parameter version). */
typedef struct ace_hpx_weight ace_hpx_weight;
int ace_hpx_weight_create(const float* w_dev, int rows, int cols, void* stream, ace_hpx_weight** out);
void ace_hpx_weight_destroy(ace_hpx_weight* w);
/* nn.Conv2d(k, dilation, padding 0) on already padded faces (+ bias, + residual, activation 0 none / 1 GELU(erf) / 2 ReLU,
 * clamped from above by `cap`: CappedGELU healpix_activations.py:41-85; cap = +inf: none) as ONE contraction over
 * (tap, channel).  x: [imgs][cin][H + (k-1) dil][pitch]; optional second source x2 (channels cin .. cin + cin2 - 1) and
 * residual R with k = 1 only; w: prepared from [cout][(ky k + kx) (cin + cin2) + i]; row_off (k > 1, device): element
 * offset of contraction row (tap, i) = ky dil pitch + kx dil + i (H + (k-1) dil) pitch; R / y: [imgs][cout][H][pitch].
 * xmax / x2max: bound slots of the sources; ymax (optional): bound slot of y. */
int ace_hpx_conv(const float* x, const float* x2, int cin, int cin2, const ace_hpx_weight* w, const long* row_off, const float* bias,
                 const float* R, float* y, int imgs, int cout, int H, int W, int pitch, int k, int dil, int act, float cap,
                 const unsigned* xmax, const unsigned* x2max, unsigned* ymax, void* stream);
/* The k x k (k >= 2) convolutions on the packed-operand engine: ace_hpx_pad_planes does the face padding of x (and, for the skip
 * concatenation, x2 behind it) straight into the engine's activation format - fp16 hi / lo planes [imgs][cpad / 8][(nside + 2 p) x
 * y_pitch cells][8 channels], cpad = channels rounded up to 8, scaled by the bound it publishes to pmax (+ ACE_HPX_SLACK_FLOATS
 * zero ENTRIES of 16 bytes behind each of hi, lo, kept allocated by the caller) - and ace_hpx_conv_packed contracts it with a weight
 * prepared from [cout][(ky k + kx) cpad + i] (zero columns for i >= channels).  Same arithmetic as ace_hpx_conv (compensated fp16,
 * fp32 accumulation), results equal to rounding; both operands stream by LDS-DMA. */
int ace_hpx_pad_planes(const float* x, long x_img_stride, long x_chan_stride, int x_pitch, const float* x2, long x2_img_stride,
                       long x2_chan_stride, int x2_pitch, int cin, int cin2, void* hi, void* lo, const int* idx_a_dev, const int* idx_b_dev,
                       int items, int nside, int p, int y_pitch, const unsigned* xmax, const unsigned* x2max, unsigned* pmax, void* stream);
int ace_hpx_conv_packed(const void* xhi, const void* xlo, int cpad, long x_plane_cells, const ace_hpx_weight* w, const float* bias,
                        float bias_max, float* y, void* yhi, void* ylo, long y_plane_cells, int imgs, int cout, int H, int W, int pitch, int k,
                        int dil, int act, float cap, const unsigned* pmax, unsigned* ymax, void* stream);
/* ... whose result may (also / instead: y NULL) be written in the same format - yhi / ylo: [imgs][cout / 8][H pitch][8], cout % 8 == 0,
 * scaled by the bound winf max|x| + bias_max (bias_max = max |bias|; <= cap for a capped activation) published to ymax - for a 1 x 1
 * convolution that follows (ConvNeXt: 3 x 3 -> GELU -> 1 x 1): ace_hpx_conv1_packed reads it (+ bias, + residual R, activation without a
 * cap), so the widest activation of the block never exists in fp32.
 * x_plane_cells / y_plane_cells (0: the natural sizes): entries per channel-group plane when xhi / yhi point at a shifted origin inside
 * the planes of a larger padded tensor: k = 1 reading the interior of planes padded for a k x k convolution (the ConvNeXt skip
 * convolution shares the block's padded input), or a k x k result written into the interior of the NEXT convolution's padded planes,
 * whose halo ace_hpx_halo_planes then gathers in place from the neighbouring faces' interiors (no second padding pass). */
int ace_hpx_halo_planes(void* hi, void* lo, int cpad, const int* idx_a_dev, const int* idx_b_dev, int items, int nside, int p, int y_pitch,
                        void* stream);
int ace_hpx_conv1_packed(const void* xhi, const void* xlo, int cin, const ace_hpx_weight* w, const float* bias, const float* R, float* y,
                         int imgs, int cout, int H, int W, int pitch, int act, const unsigned* xslot, unsigned* ymax, void* stream);
/* nn.AvgPool2d(2) / nn.MaxPool2d(2) on `planes` = imgs * channels planes (the input's bound also bounds the result). */
int ace_hpx_pool2(const float* x, float* y, long planes, int H, int W, int pitch_in, long plane_stride_in, int pitch_out,
                  long plane_stride_out, int is_max, void* stream);
/* nn.Upsample(scale_factor=2, mode) on `planes` planes (healpix_blocks.py:197-252 "Interpolate", 699-759 SmoothedInterpolate's resize):
 * mode 0 "nearest", 1 "bilinear" (align_corners as torch defines it).  y: [planes][2 H][pitch_out].  The input's bound also bounds the result. */
int ace_hpx_upsample2(const float* x, float* y, long planes, int H, int W, int pitch_in, long plane_stride_in, int pitch_out,
                      long plane_stride_out, int mode, int align_corners, void* stream);
/* nn.ConvTranspose2d(cin, cout, 2, stride 2) + activation (healpix_blocks.py:636-697).  w: prepared from
 * [(dy 2 + dx) cout + o][cin]; tmp: imgs * 4 cout * H * pitch_in floats of scratch; y: [imgs][cout][2 H][pitch_out]. */
int ace_hpx_tconv2(const float* x, const ace_hpx_weight* w, const float* bias, float* tmp, float* y, int imgs, int cin, int cout, int H,
                   int W, int pitch_in, int pitch_out, long plane_stride_out, int act, float cap, const unsigned* xmax, unsigned* ymax,
                   void* stream);


/* ------------------------------------------------------------------------------------------
 * Lat-lon UNet glue (the Samudra ocean emulator, fme/ace/models/ocean/m2lines/): activations are [img][channel][H][pitch] fp32
 * (pitch >= W; gap columns [W, pitch) defined) with a bound slot as above; the convolutions are ace_hpx_conv_packed /
 * ace_hpx_conv1_packed on the P-format planes ace_ll_pad_planes writes.  Stream-ordered; no allocation or host synchronisation.
 * ------------------------------------------------------------------------------------------ */
const char* ace_ll_last_error(void);   /* as ace_last_error(): one message per thread for the whole library */
/* hi / lo [imgs][cpad / 8][(H + 2p) x pitch_p cells][8] (cpad = c rounded up to 8, the extra channels zero; + ACE_HPX_SLACK_FLOATS zero
 * entries behind each, kept allocated by the caller) <- the halo-padded act(scale x + shift): longitude circular (circular = 1, p <= W)
 * or zero, latitude zero, gap columns [W + 2p, pitch_p) zero.  ss (optional): (scale, shift) float pairs at ss[2 (img ss_img_stride + ch)]
 * (ss_img_stride 0: one pair per channel).  act 0 none / 1 GELU(erf) clamped from above at cap.  The planes are scaled by the bound
 * act_bound(bscale bound(xmax) + boff) published to pmax (xmax: bound of the affine's input, or of its output with bscale 1, boff 0);
 * after a capped GELU the bound is max(min(cap, b), 0.17).  p = 0: the operand of a 1 x 1 convolution. */
int ace_ll_pad_planes(const float* x, long x_img_stride, long x_chan_stride, int x_pitch, int c, int H, int W, int p, int circular,
                      void* hi, void* lo, int pitch_p, int imgs, const float* ss, long ss_img_stride, int act, float cap,
                      const unsigned* xmax, float bscale, float boff, unsigned* pmax, void* stream);
/* Instance-norm statistics of the H x W interior of every (img, channel) plane: mean and biased variance (two passes, fp64
 * accumulation of (x - mean)^2), emitted as ss[2 plane] = gamma / sqrt(var + eps), ss[2 plane + 1] = beta - mean scale
 * (gamma / beta optional, per channel); mean_var (optional): (mean, var) pairs; amax: bound slot of the normalised planes. */
int ace_ll_norm_stats(const float* x, long img_stride, long chan_stride, int pitch, int imgs, int c, int H, int W, float eps,
                      const float* gamma, const float* beta, float* ss, float* mean_var, unsigned* amax, void* stream);
/* nn.AvgPool2d(2) with floor at odd H / W: y [planes][H / 2][pitch_out] (gap columns zeroed); amax: bound slot of y. */
int ace_ll_pool2(const float* x, float* y, long planes, int H, int W, int pitch_in, long plane_stride_in, int pitch_out,
                 long plane_stride_out, unsigned* amax, void* stream);
/* y [planes][H][pitch_y] = pad(Upsample(x2, bilinear, align_corners false)) + skip: x [planes][h][pitch_x] interpolated to 2h x 2w
 * (periodic = 1: periodic in longitude - the reference's ZonallyPeriodicBilinearUpsample), then padded to the skip's H x W by
 * ((H - 2h) / 2, rest) rows of zeros and ((W - 2w) / 2, rest) columns, circular (circular = 1) or zero; amax: bound slot of y. */
int ace_ll_upsample2_add(const float* x, long planes, int h, int w, int pitch_x, long plane_stride_x, const float* skip, int pitch_skip,
                         long plane_stride_skip, float* y, int H, int W, int pitch_y, long plane_stride_y, int circular, int periodic,
                         unsigned* amax, void* stream);

/* ------------------------------------------------------------------------------------------
 * Ocean corrector (fme/core/corrector/ocean.py, "ocean_corrector"): force positive -> sea-ice fraction clamp / rebalance /
 * zeroing -> surface energy flux (hfds) correction -> ocean heat content budget, in place on the output planes of one step.
 * Two launches: O1 (one column per thread: every column-local correction, the columns' heat contents and net flux into the
 * ocean, fp64 partial sums per workgroup of the masked area-weighted means), O2 (per sample: the partials re-summed in a
 * fixed order, the ratio in fp64, every thetao level and the SST scaled).  No atomics, no allocation, no host
 * synchronisation; input and forcing planes are only read.  Planes: ace_phys_plane, p = NULL means "absent".
 * ------------------------------------------------------------------------------------------ */
#define ACE_OCEAN_MAX_LEVELS 64
#define ACE_OCEAN_MAX_POSITIVE 40
#define ACE_OCEAN_MAX_ZERO 8

typedef struct ace_ocean_config {
    int nlat, nlon;
    int nlev;                          /* depth layers (the dz table has nlev planes); 0 without the heat-content correction */
    int max_batch;
    int sea_ice;                       /* SeaIceFractionConfig present */
    int remove_negative_ocean_fraction;
    int hfds;                          /* 0 none, 1 "residual_prediction", 2 "prescribed" */
    int ohc;                           /* 0 none, 1 "scaled_temperature" */
    double timestep_seconds;
    double unaccounted_heating;        /* OceanHeatContentBudgetConfig.constant_unaccounted_heating */
} ace_ocean_config;

typedef struct ace_ocean_fields {
    /* output of the step, corrected in place */
    ace_phys_plane positive[ACE_OCEAN_MAX_POSITIVE];   /* force_positive_names */
    int npositive;
    ace_phys_plane sif;                            /* sea_ice_fraction_name */
    ace_phys_plane zero[ACE_OCEAN_MAX_ZERO];       /* zero_where_ice_free_names */
    int nzero;
    ace_phys_plane hfds;                           /* hfds, or hfds_total_area (hfds_total_area = 1) */
    int hfds_total_area;
    ace_phys_plane thetao[ACE_OCEAN_MAX_LEVELS];   /* thetao_0 .. thetao_{nlev-1} */
    ace_phys_plane sst;                            /* optional */
    /* input of the step (read only) */
    ace_phys_plane reb_land;                       /* input[land_fraction_name] of the sea-ice rebalance */
    ace_phys_plane in_land, in_sif, in_sst;        /* ocean fraction 1 - land - sif; sst of the net flux */
    int in_sif_is_ocean_sif;                       /* in_sif is ocean_sea_ice_fraction: sif = it * (1 - land) */
    ace_phys_plane thetao_in[ACE_OCEAN_MAX_LEVELS];
    ace_phys_plane in_flux, in_ssf;                /* heat-budget flux from the input (flux_source 2 / 3) */
    int in_ssf_is_land;                            /* in_ssf holds land_fraction: ssf = 1 - it */
    int flux_source;                               /* 0 output hfds_total_area, 1 output hfds, 2 input hfds,
                                                      3 input hfds_total_area / input sea-surface fraction */
    /* next step's forcing (read only) */
    ace_phys_plane dlw, ulw, dsw, usw, lhf, shf, precip;
    ace_phys_plane frozen, frozen_parts[3];        /* total_frozen_precipitation_rate, or ICE + GRAUPEL + SNOW; absent: 0 */
    ace_phys_plane f_ssf;                          /* sea_surface_fraction, or land_fraction (f_ssf_is_land = 1) */
    int f_ssf_is_land;
    ace_phys_plane hfgeou;                         /* optional: absent is 0 */
} ace_ocean_fields;

typedef struct ace_ocean_phys ace_ocean_phys;
const char* ace_ocean_phys_last_error(void);   /* as ace_last_error(): one message per thread for the whole library */
/* area_weights_lat_host: nlat fp32 weights per row; dz_host: (nlev, nlat, nlon) fp32 layer thicknesses (DepthCoordinate.dz,
 * zero where masked); mask_ohc_host: (nlat, nlon) fp32 mask the provider gives for "ocean_heat_content" (NULL: none);
 * mask0_host: (nlat, nlon) fp32 top-level ocean mask (heat content is NaN where it is 0).  All but the first may be NULL
 * without the heat-content correction. */
int ace_ocean_phys_create(const ace_ocean_config* cfg, const float* area_weights_lat_host, const float* dz_host,
                          const float* mask_ohc_host, const float* mask0_host, ace_ocean_phys** out);
void ace_ocean_phys_destroy(ace_ocean_phys* h);
/* One step; `fields` is a HOST struct of device planes (copied into the kernel arguments). */
int ace_ocean_phys_apply(ace_ocean_phys* h, const ace_ocean_fields* fields, int batch, void* stream);
/* Route query: O1 / O2 launches this handle has made. */
int ace_ocean_phys_launches(const ace_ocean_phys* h, long* o1, long* o2);

/* ------------------------------------------------------------------------------------------
 * The ocean's derived variables (fme/core/ocean_derived_variables.py; OceanData, fme/core/ocean_data.py) over one window of
 * batch x steps x hw pixels, any subset of the seven in one launch.  Every input plane is read once, every wanted output
 * written once; no atomics, no scratch, no allocation, no host synchronisation; all fp64 work in a fixed order, so two
 * identical calls - and calls that differ in t_chunk only - give identical bytes.
 *
 * A field is {base, bstride, tstride}: the plane of sample b at step t is the hw contiguous floats at base + b * bstride +
 * t * tstride (strides in floats, any 4-byte alignment; tstride 0 is a field constant in time); base NULL: absent.  A thetao
 * level carries in addition `head`, the plane of the time level before step 0 (the initial condition) at head + b *
 * head_bstride; NULL: the initial condition has no such level.  dz is (nlev, hw) fp32 (DepthCoordinate.dz, 0 where masked),
 * mask0 (hw) fp32 the top level's ocean mask, area_m2 (hw) fp32 the cell areas in square metres (HI only; else NULL).
 * Name resolution is the host's job: which of the reference's alternatives applies follows from which planes are present.
 *
 * With CP_RHO = 3992.0 * 1035.0 (SPECIFIC_HEAT_OF_SEA_WATER_CM4 * DENSITY_OF_SEA_WATER_CM4) as one double and ssf the
 * sea_surface_fraction plane, or 1 - land_fraction in fp32 when that is absent:
 *   S(b, t, p)   CP_RHO * sum over k = 0 .. nlev - 1, in that order, of (double) thetao_k * (double) dz_k(p) in fp64 (every product
 *                is exact), a NaN thetao_k contributing 0 (the reference's nansum); S(b, -1, p) is the same sum over the head
 *                planes, an absent head plane counting as NaN
 *   OHC          ocean_heat_content: (float) S where mask0(p) > 0, NaN elsewhere
 *   OHC_TENDENCY ocean_heat_content_tendency: where mask0(p) > 0, (float) ((S_t - S_{t-1}) / dt_seconds), the difference taken on
 *                the fp64 sums; NaN where mask0(p) <= 0; at t = 0 without has_head +0.0 everywhere, land included (the
 *                reference's zeros_like row)
 *   HFDS         hfds (only when the hfds plane is absent): hfds_total_area / ssf, the correctly rounded fp32 quotient
 *   NET_FLUX     net_energy_flux_into_ocean_column: (hfds + hfgeou) * ssf in fp32, in that order; hfds the plane or the
 *                quotient above; an absent hfgeou is +0.0
 *   ADVECTION    implied_tendency_of_ocean_heat_content_due_to_advection: the fp32 tendency as output minus the net flux, fp32
 *   SEA_ICE_FRACTION  sea_ice_fraction (only when that plane is absent): ocean_sea_ice_fraction * (1 - land_fraction) in fp32
 *   HI           sea-ice thickness: with frac = ocean_sea_ice_fraction * ssf, or (sea_ice_fraction * ssf) / (1 - land_fraction)
 *                when ocean_sea_ice_fraction is absent, both in fp32, and vol = sea_ice_volume, area = area_m2:
 *                (double) vol * 1e9 / ((double) area * (double) frac) in fp64 (both products exact), rounded to fp32.  At
 *                special inputs it has the value of the reference's where(isnan(vol), NaN, nan_to_num(exp(9 ln 10 + ln vol -
 *                ln area - ln frac))) on the extended reals, the first matching row of
 *                    vol NaN                                   NaN
 *                    frac, area or 1 - land_fraction NaN       0
 *                    vol < 0, frac < 0 or area < 0             0
 *                    vol == 0, whatever frac                   0
 *                    frac == +inf or area == +inf              0
 *                    vol == +inf                               FLT_MAX
 *                    vol > 0 and frac == 0 (or area == 0)      FLT_MAX
 *                    any overflow past FLT_MAX                 FLT_MAX
 * Output i of `want` (bit 1 << i, i one of ACE_OCEAN_DERIVE_*) is written at out[i] + b * out_bstride + t * out_tstride; of an
 * output not in `want` not one byte is touched, and its out[i] is not read.
 *
 * Time is cut into chunks of t_chunk steps (0: chosen by the library so that a small window still fills the device); a
 * chunk's first step recomputes S of the step before it, so chunks are independent.
 *
 * Refused (ACE_ERR_INVALID before any launch, the reason behind ace_ocean_derive_last_error, nothing written): a wanted output
 * with an absent input (for OHC, OHC_TENDENCY and ADVECTION: dz, mask0 and every thetao_k, k < nlev, with nlev in 1 ..
 * ACE_OCEAN_MAX_LEVELS; dt_seconds > 0 for the latter two) or a NULL destination; HFDS or SEA_ICE_FRACTION wanted while its
 * plane exists; nlev outside 0 .. ACE_OCEAN_MAX_LEVELS whatever is wanted; batch outside 1 .. 65535, steps < 1, hw < 1,
 * t_chunk < 0, more than 65535 time chunks; bits of `want` above the seven.  want == 0 is a no-op.
 * ------------------------------------------------------------------------------------------ */
#define ACE_OCEAN_DERIVE_OHC 0                 /* the reference's registration order */
#define ACE_OCEAN_DERIVE_OHC_TENDENCY 1
#define ACE_OCEAN_DERIVE_ADVECTION 2
#define ACE_OCEAN_DERIVE_NET_FLUX 3
#define ACE_OCEAN_DERIVE_SEA_ICE_FRACTION 4
#define ACE_OCEAN_DERIVE_HI 5
#define ACE_OCEAN_DERIVE_HFDS 6
#define ACE_OCEAN_DERIVE_NOUT 7

typedef struct ace_ocean_derive_field { const float* base; long bstride, tstride; } ace_ocean_derive_field;
typedef struct ace_ocean_derive_level { ace_ocean_derive_field f; const float* head; long head_bstride; } ace_ocean_derive_level;

typedef struct ace_ocean_derive_desc {
    int nlev;
    ace_ocean_derive_level thetao[ACE_OCEAN_MAX_LEVELS];
    const float* dz;
    const float* mask0;
    const float* area_m2;
    ace_ocean_derive_field hfds, hfds_total_area, hfgeou, sea_surface_fraction, land_fraction, ocean_sea_ice_fraction,
        sea_ice_fraction, sea_ice_volume;
    float* out[ACE_OCEAN_DERIVE_NOUT];
    long out_bstride, out_tstride;
    unsigned want;
    int has_head;
    double dt_seconds;
    int batch, steps;
    long hw;
    int t_chunk;
} ace_ocean_derive_desc;

const char* ace_ocean_derive_last_error(void);   /* as ace_last_error(): one message per thread for the whole library */
/* `desc` is a HOST struct of device pointers (copied into the kernel arguments). */
int ace_ocean_derive_window(const ace_ocean_derive_desc* desc, void* stream);

/* ------------------------------------------------------------------------------------------
 * Sea-ice budget corrector (fme/core/corrector/ice.py, "ice_corrector": IceBudgetCorrectionConfig).  For each of up to three
 * variables v, in the order given (the reference's: simass, the concentration, sisnmass), the three budget terms of the step's
 * output (source, sink, transport: planes corrected in place) are rebalanced so that the new mass old + dt * (s + k + t) is not
 * negative, not above 1 (area_mode) and zero where there is no ice (masked), and the output's prognostic plane is overwritten
 * with that mass.  `old` is the input's plane of the variable and is only read.
 *
 * Per pixel, everything in fp64, every operation rounded on its own (no fused multiply-add), with dt = timestep:
 *   s = (double) source * dt, k = (double) sink * dt, t = (double) transport * dt, o = (double) old
 *   new(s, k, t) = o + ((s + k) + t)
 *   rebalance(s, k, t, m, mass, sign), m the pixel's stage mask, mass = 0 where m is false:
 *       nz_x = |x| > 0 for x in s, k, t;  n = nz_s + nz_k + nz_t;  share = (m and n > 0) ? mass / max(n, 1) : 0
 *       r_x = (m and nz_x) ? share : 0;  if (m and n == 0) r_t = mass
 *       tmp = k + sign * r_k;  ko = tmp > 0 ? tmp : 0;  r_k = r_k - ko;  r_t = r_t + ko
 *       tmp = s + sign * r_s;  so = tmp < 0 ? tmp : 0;  r_s = r_s - sign * so;  r_t = r_t + sign * so
 *       s = s + sign * r_s;  k = k + sign * r_k;  t = t + sign * r_t
 *   stage 1            m = new < 0,                      mass = -new,     sign = +1
 *   stage 2 (area_mode) m = new > 1,                     mass = new - 1,  sign = -1
 *   stage 3 (masked)    m = (ice mass == 0) and new > 0, mass = new,      sign = -1
 *   b_x = x / dt (a division);  source, sink, transport = (float) b_x;  prognostic = (float) (o + dt * ((b_s + b_k) + b_t))
 * Comparisons are IEEE: a NaN pixel enters no mask and comes out NaN.  A stage is run for EVERY pixel of the (batch, H, W)
 * tensor - where m is false it still moves a positive sink and a negative source into the transport - if and only if m is
 * true at ANY pixel of the tensor after the stages before it, and is skipped for every pixel otherwise: the reference's
 * `if torch.any(mask)`.  The "ice mass" of stage 3 is the fp64 mass of variable 0 as corrected by this call, BEFORE it is
 * rounded to fp32 (a mass that rounds to 0.0f is still ice; NaN is not zero); masked[0] must be 0.
 *
 * Contract.  A call is stream-ordered and makes no host readback, no synchronisation and no allocation: at most 2 * nvars kernel
 * launches (per variable: a flags pass that ORs, over the tensor, each pixel's stage masks under every hypothesis about the
 * earlier stages - 7 bits - and an apply pass that resolves the path from them and recomputes its pixel once along it) plus
 * one clearing of the flag words on the stream.  An OR is order-independent: two calls on the same inputs give the same bits,
 * and so do 16-byte and 4-byte plane alignments.  `scratch` is caller-owned device memory of ace_ice_budget_scratch_bytes(batch,
 * hw) bytes, 16-byte aligned, that must not be shared by calls in flight on different streams: flag words, then one byte per
 * pixel (the fp64 "ice mass == 0" predicate of variable 0).  Every plane holds `batch` samples of H * W contiguous floats.
 *
 * Refused (ACE_ERR_INVALID before any launch, the reason behind ace_ice_budget_last_error, nothing written): NULL fields or
 * scratch (with nvars > 0), nvars outside 0 .. ACE_ICE_MAX_VARS, an absent plane, masked[0] set, a timestep that is not a
 * positive finite number, batch outside 1 .. 65535, H or W < 1, a scratch that is not 16-byte aligned.  nvars == 0 is a no-op.
 * ------------------------------------------------------------------------------------------ */
#define ACE_ICE_MAX_VARS 3
#define ACE_ICE_FLAG_BYTES 64                  /* head of the scratch: one 32-bit flag word per variable, padded */

typedef struct ace_ice_var {
    ace_phys_plane old_mass;                   /* input of the step (read only) */
    ace_phys_plane source, sink, transport;    /* output of the step, corrected in place */
    ace_phys_plane mass;                       /* output of the step, overwritten */
    int area_mode;                             /* a concentration: capped at 1 */
    int masked;                                /* zero where variable 0's corrected mass is zero */
} ace_ice_var;

typedef struct ace_ice_fields {
    ace_ice_var var[ACE_ICE_MAX_VARS];
    int nvars;
} ace_ice_fields;

const char* ace_ice_budget_last_error(void);   /* as ace_last_error(): one message per thread for the whole library */
long ace_ice_budget_scratch_bytes(int batch, long hw);
/* `fields` is a HOST struct of device planes (copied into the kernel arguments). */
int ace_ice_budget_apply(const ace_ice_fields* fields, double timestep, int batch, int H, int W, void* scratch, void* stream);
/* Launch counter of this process: flags passes, apply passes and flag clearings enqueued so far (any may be NULL). */
int ace_ice_budget_launches(long* flags, long* apply, long* clears);

/* ------------------------------------------------------------------------------------------
 * Per-pixel MLP (csrc/pixel_mlp.hip): a chain of 1 x 1 convolutions - the LandNet family, fme/ace/models/land/land_net.py - as
 * one launch per forward in exact fp32 (v_mfma_f32_16x16x4_f32), the hidden activations staying in registers.
 *
 * create(n_layers, dims[n_layers + 1], w_dev[], bias_dev[], act[], embed_layer, stream, &handle) reads the DEVICE weights
 * (w_dev[l]: row-major [dims[l + 1]][dims[l]] fp32; bias_dev NULL or bias_dev[l] NULL: no bias; act[l] one of ACE_PIXEL_MLP_ACT_*)
 * once, synchronising `stream`, into one device blob in the kernel's fragment order; the handle does not refer to the caller's
 * arrays afterwards (a changed weight needs a new handle).  embed_layer: the layer after whose activation a plane stack
 * [dims[embed_layer + 1]][hw] is added, -1 for none.
 * forward(handle, x, embed, y, batch, hw, stream): x [batch][dims[0]][hw], y [batch][dims[n_layers]][hw], embed
 * [dims[embed_layer + 1]][hw] (ignored without an embedding layer), contiguous fp32, x and y not overlapping.  One launch,
 * stream-ordered, no allocation, no host synchronisation: capturable.
 *
 * The statement (tests/_pixel_mlp_ref.py is this text in numpy).  Per pixel, a = the dims[0] inputs; per layer l with
 * K = dims[l], O = dims[l + 1], for every o < O:
 *     acc = bias[l][o] (+0.0f without a bias)
 *     for t in 0 .. ceil(K / 16) - 1:  for r in 0 .. 3:  for g in 0 .. 3:
 *         k = 16 t + 4 g + r;  if k < K:  acc = fmaf(w[l][o][k], a[k], acc)
 *     if act[l] == ACE_PIXEL_MLP_ACT_RELU:  acc = acc < 0 ? +0.0f : acc         (torch.relu: NaN stays NaN, -0.0f stays -0.0f)
 *     if l == embed_layer:  acc = acc + embed[o][pixel]                         (one fp32 addition)
 *     a'[o] = acc
 * Every layer, the first included, uses that k order (the order in which an MFMA accumulator tile is the next MFMA's operand).
 * fmaf is the single-rounding fused multiply-add; nothing else is fused (contraction is off in the translation unit) and
 * subnormals are kept.  Channel padding up to the 16-wide tile contributes nothing, also beside Inf or NaN: a padded
 * activation is forced to +0.0f and meets a padded weight of -0.0f, and x + (-0.0f) == x bit for bit for every x.  A pixel's
 * result depends on that pixel only.
 *
 * Any hw >= 1 and any 4-byte alignment are accepted.  Widths up to ACE_PIXEL_MLP_NARROW_WIDTH: a wave carries
 * ACE_PIXEL_MLP_NARROW_TILES tiles of ACE_PIXEL_MLP_TILE pixels, with 16-byte accesses when hw % 4 == 0 and x, y and embed are
 * 16-byte aligned (one decision for the launch), 4-byte ones otherwise; wider chains carry ACE_PIXEL_MLP_WIDE_TILES tile.  A
 * workgroup is ACE_PIXEL_MLP_WAVES waves, one (sample, run of pixels) unit per wave and pass; at most ACE_PIXEL_MLP_MAX_GRID
 * workgroups are launched, so a workgroup loops once batch * ceil(hw / (tiles * ACE_PIXEL_MLP_TILE)) exceeds
 * ACE_PIXEL_MLP_MAX_GRID * ACE_PIXEL_MLP_WAVES.  The weight blob - per layer ceil(O / 16) * 16 bias floats and
 * ceil(O / 16) * ceil(K / 16) * 256 fragment floats - is copied into LDS once per workgroup when it is at most
 * ACE_PIXEL_MLP_LDS_BYTES and read from global memory, fragment by fragment, otherwise; both kernels have both forms and the
 * arithmetic does not depend on the form.
 *
 * Refused (ACE_ERR_INVALID, the reason behind ace_pixel_mlp_last_error, nothing launched): a NULL handle, x or y; batch < 1;
 * hw < 1; embed NULL where the handle has an embedding layer; in create: n_layers outside 1 .. ACE_PIXEL_MLP_MAX_LAYERS, a
 * width outside 1 .. ACE_PIXEL_MLP_MAX_WIDTH, a NULL weight, an unknown activation, embed_layer outside -1 .. n_layers - 1.
 * ------------------------------------------------------------------------------------------ */
#define ACE_PIXEL_MLP_MAX_LAYERS 8
#define ACE_PIXEL_MLP_MAX_WIDTH 256
#define ACE_PIXEL_MLP_ACT_NONE 0
#define ACE_PIXEL_MLP_ACT_RELU 1
#define ACE_PIXEL_MLP_ACT_GELU 2               /* 0.5 v (1 + erff(v / sqrt 2)): nn.GELU(); held to torch's fp32 error, not to bits */
#define ACE_PIXEL_MLP_ACT_SILU 3               /* v / (1 + expf(-v)): nn.SiLU(); likewise */
#define ACE_PIXEL_MLP_TILE 16                  /* pixels of one MFMA tile */
#define ACE_PIXEL_MLP_WAVES 4                  /* waves of a workgroup */
#define ACE_PIXEL_MLP_NARROW_WIDTH 64          /* every width <= this: the narrow kernel */
#define ACE_PIXEL_MLP_NARROW_TILES 4           /* pixel tiles per wave, narrow */
#define ACE_PIXEL_MLP_WIDE_TILES 1             /* pixel tiles per wave, wide */
#define ACE_PIXEL_MLP_MAX_GRID 512             /* workgroups of a launch */
#define ACE_PIXEL_MLP_LDS_BYTES 65536          /* a weight blob up to this size is copied into LDS, a larger one streamed from global memory */

const char* ace_pixel_mlp_last_error(void);   /* as ace_last_error(): one message per thread for the whole library */
int ace_pixel_mlp_create(int n_layers, const int* dims, const float* const* w_dev, const float* const* bias_dev, const int* act,
                         int embed_layer, void* stream, void** handle);
void ace_pixel_mlp_destroy(void* handle);
int ace_pixel_mlp_forward(void* handle, const float* x, const float* embed, float* y, int batch, long hw, void* stream);
/* create with one more argument: embed_before_act != 0 moves the embedding's addition in front of the activation of layer
 * embed_layer (acc = act(acc + embed[o][pixel]): AnkurLocalNet's Conv2d -> AddPosEmbed -> activation), and act[l] may also be
 * ACE_PIXEL_MLP_ACT_GELU or ACE_PIXEL_MLP_ACT_SILU (create goes on refusing them).  On what create accepts, create2(..., 0) is
 * create: the same blob, the same kernels, the same bytes - a chain of none / ReLU with the embedding after the activation runs the
 * instantiations it ran before these options existed.  An embed_before_act other than 0 or 1 is refused. */
int ace_pixel_mlp_create2(int n_layers, const int* dims, const float* const* w_dev, const float* const* bias_dev, const int* act,
                          int embed_layer, int embed_before_act, void* stream, void** handle);

/* ------------------------------------------------------------------------------------------
 * DISCO convolution on the sphere (csrc/disco.hip): the first layer of AnkurLocalNet (fme/core/models/conditional_sfno/ankur.py)
 * and the filter of LocalNet's "disco" blocks (fme/core/disco/_convolution.py) - the contraction of the input with the sparse psi
 * table, the grouped mix with the weight, an optional positional embedding and the activation - as ONE launch in exact fp32.  The
 * reference goes through rfft, a banded einsum, irfft and a grouped einsum; the operator itself is a short sum per output pixel.
 *
 * create(H, W, K, row_off, hi, wi, vals, w_dev, in_chans, out_chans, groups, act, has_embed, stream, &handle): the psi table
 * (ace_amd/disco.py) in HOST memory - row_off [H + 1] (long), and per support point the input row hi, the input column wi at
 * output column 0 (ascending (hi, wi) within an output row) and K fp32 values vals[point][k]; the DEVICE weight w_dev
 * [out_chans][in_chans / groups][K], read once, synchronising `stream`.  K = ks * ks, ks = 1 .. 5.  groups divides in_chans and
 * out_chans (the reference passes their gcd).  act: ACE_DISCO_ACT_*.  create builds one device blob (row records, point offsets,
 * psi, the unit list, the weight in MFMA fragment order) and the unit list (csrc/disco_units.h) once; the handle does not refer
 * to the caller's arrays afterwards.
 * forward(handle, x, embed, y, batch, stream): x [batch][in_chans][H][W], y [batch][out_chans][H][W], embed [out_chans][H][W]
 * (ignored when has_embed == 0), contiguous fp32, any 4-byte alignment, x and y not overlapping.  One launch, stream-ordered, no
 * allocation, no host synchronisation, no atomics: capturable, and two runs are bitwise identical.
 * info(handle, out[4]): units of a launch per sample, the heaviest unit's cost, the cost of all units, the launch's LDS bytes.
 *
 * The statement (tests/_disco_ref.py is this text in numpy).  Exact fp32; per sample b, output row ho, output column wo, with
 * gs = in_chans / groups and opg = out_chans / groups:
 *     for c < in_chans, k < K:
 *         z[c][k] = +0.0f
 *         for e over the points of row ho in table order:
 *             z[c][k] = fmaf(vals[e][k], x[b][c][hi_e][(wi_e + wo) mod W], z[c][k])
 *     for o < out_chans, with g = o / opg:
 *         acc = +0.0f
 *         for j = 0 .. gs * K - 1, in ascending order, j = c' * K + k:
 *             acc = fmaf(w[o][c'][k], z[g * gs + c'][k], acc)
 *         if has_embed:  acc = acc + embed[o][ho][wo]                 (before the activation, as AddPosEmbed stands in the net)
 *         y[b][o][ho][wo] = act(acc)
 * fmaf is the single-rounding fused multiply-add; nothing else is fused and subnormals are kept.  Activations: NONE; RELU
 * acc < 0 ? +0.0f : acc (NaN stays NaN, -0.0f stays -0.0f); GELU 0.5 acc (1 + erff(acc / sqrt 2)); SILU acc / (1 + expf(-acc)) -
 * the last two with this toolchain's erff / expf, held to torch's own fp32 error and not to bits.  A point whose value is exactly
 * 0 is a term like any other: 0 * Inf is NaN.  A NaN or Inf at x[b][c][p] reaches exactly the outputs of c's group whose support
 * holds p: groups are contracted one by one (no block-diagonal weight), and the padding of gs * K up to a multiple of 4 meets a
 * +0.0f z row with a -0.0f weight, an identity of the chain.
 *
 * A workgroup (ACE_DISCO_WAVES waves) owns one unit (sample, output row, run of up to ACE_DISCO_RUN output columns, run of
 * groups): it stages the band rows of its channels in LDS (at most ACE_DISCO_STAGE_BYTES per pass, more channels in further
 * passes), forms z with psi values that are uniform across the wave - one LDS read per K multiply-adds - into at most
 * ACE_DISCO_Z_BYTES of LDS, contracts it with the group's weight on v_mfma_f32_16x16x4_f32 and writes y once; z never goes to
 * memory.  Units are listed on the host, heaviest first; a polar row, whose disk wraps every longitude, is split over groups and
 * then over shorter pixel runs (down to ACE_DISCO_MIN_RUN) until a unit costs no more than 1 / ACE_DISCO_TARGET_UNITS of a sample
 * (or ACE_DISCO_MIN_UNIT_COST, if that is more).
 * Accepted: W below or no multiple of the run, gs * K no multiple of 4, opg from 1 (depthwise) up, groups == 1.
 *
 * Refused (ACE_ERR_INVALID, the reason behind ace_disco_last_error, nothing launched): a NULL handle, x or y; batch < 1; embed
 * NULL where has_embed; batch * units beyond 2^31 - 1; in create: a NULL argument, K not ks * ks with ks in 1 .. 5
 * (ACE_DISCO_MAX_K), groups not dividing both channel counts, gs * K over ACE_DISCO_MAX_PRODUCTS, an unknown activation, an
 * output row without a point, a point outside the grid, points out of order, one channel's band over ACE_DISCO_STAGE_BYTES.
 * ------------------------------------------------------------------------------------------ */
#define ACE_DISCO_ACT_NONE 0
#define ACE_DISCO_ACT_RELU 1
#define ACE_DISCO_ACT_GELU 2
#define ACE_DISCO_ACT_SILU 3
#define ACE_DISCO_MAX_K 25                     /* basis functions: kernel_size <= 5 */
#define ACE_DISCO_MAX_PRODUCTS 512             /* (in_chans / groups) * K */
#define ACE_DISCO_RUN 16                       /* output columns of a unit: the pixel side of the MFMA tile */
#define ACE_DISCO_MIN_RUN 4                    /* the shortest run a polar row is split into */
#define ACE_DISCO_WAVES 4                      /* waves of a workgroup */
#define ACE_DISCO_STAGE_BYTES 65536            /* LDS of the staged band rows of one pass */
#define ACE_DISCO_Z_BYTES 32768                /* LDS of a unit's z: groups * roundup4(gs * K) * ACE_DISCO_RUN floats */
#define ACE_DISCO_TARGET_UNITS 2048            /* a unit costs at most 1 / this of a sample's work, where the split allows ... */
#define ACE_DISCO_MIN_UNIT_COST 4096           /* ... but a unit at or below this many (point, pixel, channel) products is not split */

const char* ace_disco_last_error(void);   /* as ace_last_error(): one message per thread for the whole library */
int ace_disco_create(int H, int W, int K, const long* row_off, const int* hi, const int* wi, const float* vals, const float* w_dev,
                     int in_chans, int out_chans, int groups, int act, int has_embed, void* stream, void** handle);
void ace_disco_destroy(void* handle);
int ace_disco_forward(void* handle, const float* x, const float* embed, float* y, int batch, void* stream);
int ace_disco_info(void* handle, long* out4);

#ifdef __cplusplus
}
#endif
#endif /* ACE_SFNO_H */
