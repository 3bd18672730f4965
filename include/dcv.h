/*
 * dcv.h -- C-ABI of libdcv.so, the MI355X (gfx950) engine behind deep_cartograph's CV-fit
 * hot path (train_colvars: pca / tica / htica / ae / deep_tica / vae, projection, k-means).
 *
 * The reference has no FFI for this path: the seam is the Python class set in
 * deep_cartograph/modules/cv_learning/cv_calculator.py and the functions of
 * deep_cartograph/modules/statistics/statistics.py.  Each entry point
 * below names the reference code it replaces (file:line relative to
 * /root/reference/deep_cartograph).  INTEGRATION.md shows the ctypes stub a maintainer of
 * the reference would add.
 *
 * Conventions
 *   - every function returns 0 on success, a negative DCV_E* code on failure;
 *     dcv_last_error() returns a thread-local, NUL-terminated description;
 *   - pointers named *_d are DEVICE pointers (HIP, current device), *_h are HOST pointers;
 *     the caller owns every buffer, the library never frees caller memory;
 *   - matrices are row-major; `ld` is the row stride in ELEMENTS;
 *   - `stream` is a hipStream_t passed as void* (NULL = default stream); all work is
 *     enqueued asynchronously on it, functions with *_h outputs synchronise that stream;
 *   - host arrays (*_h inputs) are taken at the call: the caller may overwrite or free them once the function has
 *     returned, whether or not it synchronised (a function that takes one may hold the host until the stream reaches it);
 *   - the library keeps no device state outside the caller's buffers and the dcv_mlp / dcv_comm handles: calls whose
 *     buffers (workspaces included) do not overlap, and calls on different dcv_mlp handles, may be in flight on different
 *     streams at the same time; one handle is driven from one stream at a time, and calls are made from one host thread
 *     at a time (the arithmetic mode, the launch-plan log and the profiling hooks are process-wide host state);
 *   - workspace sizes are queried with the matching *_workspace() call; workspaces are
 *     plain device memory with no state between calls;
 *   - one process drives one GPU; multi-GPU runs shard frames over ranks and all-reduce the
 *     small result buffers documented per call.
 */
#ifndef DCV_H
#define DCV_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DCV_OK 0
#define DCV_EINVAL (-1)  /* bad argument / unsupported shape */
#define DCV_EHIP (-2)    /* HIP runtime error */
#define DCV_ENOMEM (-3)  /* workspace too small / allocation failed */
#define DCV_ESTATE (-4)  /* call order violated */
#define DCV_ECALLBACK (-5) /* a host callback of the caller reported failure */

#define DCV_ABI_VERSION 5

int dcv_abi_version(void);
const char* dcv_last_error(void);
/* Number of compute units and bytes of device memory of HIP device `device`. */
int dcv_device_info(int device, int* n_cu, int64_t* hbm_bytes, char* name, size_t name_len);

/* Arithmetic of every matrix product of the library (time-lagged covariances, MLP forward / backward):
 *   DCV_GEMM_NATIVE_F32   v_mfma_f32_32x32x2_f32: exact f32 products, f32 accumulate (157.3 TFLOP/s peak);
 *   DCV_GEMM_SPLIT_BF16X6 each f32 operand split into three bf16 pieces (8 + 8 + 8 mantissa bits), six
 *                         v_mfma_f32_32x32x16_bf16 products per block, f32 accumulate: the dropped cross terms
 *                         are <= 2^-23 of a product, i.e. the accuracy of an f32 multiply (measured error vs
 *                         float64 at or below the native path's), on the 16x faster BF16 matrix pipe.  Default.
 * Process-wide; also settable with the environment variable DCV_GEMM_MODE=native|split before the first product. */
#define DCV_GEMM_NATIVE_F32 0
#define DCV_GEMM_SPLIT_BF16X6 1
int dcv_set_gemm_mode(int mode);
int dcv_get_gemm_mode(void);

/* ---------------------------------------------------------------- column statistics (a1)
 * Replaces DataFrame.agg(['mean','std','min','max']) in CVCalculator.load_training_data,
 * cv_calculator.py:294-297.  One pass over X (n x F float32).  `out_d` receives 4*F
 * float64: [sum | sum of squares | min | max].  Sums combine over shards by addition,
 * min/max by min/max; mean and std(ddof=1) are finalised on the host
 * (mean = sum/n, var = (sumsq - n*mean^2)/(n-1)).  Algorithmic traffic: 4*n*F bytes read. */
size_t dcv_col_stats_workspace(int64_t n, int32_t F);
int dcv_col_stats(const float* X_d, int64_t n, int32_t F, int64_t ld, double* out_d,
                  void* ws_d, size_t ws_bytes, void* stream);

/* ---------------------------------------------------------------- column histograms (filter_features)
 * Replaces np.histogram(column, bins) per feature in shannon_entropy, statistics.py:556-564.  One pass
 * over X (n x F float32).  `edges_d` holds F rows of bins + 1 float32 bin edges (built on the host as
 * np.histogram builds them from the column's min and max); `counts_d` receives F * bins int64 counts that
 * are EQUAL to np.histogram's: every bin is [edge_i, edge_i+1), the last one is closed on the right.
 * 1 <= bins <= 126.  Algorithmic traffic: 4*n*F bytes read, 8*F*bins written.  The workspace is empty
 * (the query exists for symmetry and returns 0); `ws_d` may be NULL. */
size_t dcv_col_histogram_workspace(int64_t n, int32_t F, int32_t bins);
int dcv_col_histogram(const float* X_d, int64_t n, int32_t F, int64_t ld, const float* edges_d, int32_t bins,
                      int64_t* counts_d, void* ws_d, size_t ws_bytes, void* stream);

/* ---------------------------------------------------------------- dip statistic (filter_features)
 * Replaces the statistic of diptest.diptest(column) in dip_test, statistics.py:621-632.  `Xs_d` is n x C
 * float32 with EVERY COLUMN SORTED ascending (no NaN).  `dip_d` receives C float64 dip statistics
 * (Hartigan & Hartigan 1985 / AS 217 in float64, at least 1/(2n); 0 for a constant column or n < 2),
 * `lo_d` / `hi_d` the 0-based ends of the modal interval.  n < 2^31 - 1.  The workspace holds four int32
 * arrays of (n + 1) * C.  Algorithmic traffic: two hull scans and the interval search, about
 * 4*n*C bytes read of Xs and 8*n*C bytes of hull links written per scan; latency-bound. */
size_t dcv_dip_sorted_workspace(int64_t n, int32_t C);
int dcv_dip_sorted(const float* Xs_d, int64_t n, int32_t C, int64_t ld, double* dip_d, int32_t* lo_d,
                   int32_t* hi_d, void* ws_d, size_t ws_bytes, void* stream);

/* ---------------------------------------------------------------- featurisation (compute_features)
 * Replaces the `plumed driver` subprocess of tools/compute_features/compute_features.py:200-221 and the COLVAR text it
 * writes, for the DISTANCE (NOPBC) and TORSION actions: n_frames x n_atoms x 3 float32 coordinates in, n_frames rows of
 * float32 features out.  Coordinate c of atom a in frame f is xyz_d[f*frame_stride + a*atom_stride + c*comp_stride]
 * (strides in ELEMENTS, frame_stride >= 0, the other two >= 1): a dense (n, A, 3) array has strides (3A, 3, 1); the
 * frame records of a DCD file viewed as float32 -- three planes X[A], Y[A], Z[A] between 4-byte record markers -- have
 * atom_stride 1, comp_stride A + 2 and xyz_d on the first X value, which need not be 16-byte aligned.  A frame stride
 * that is a multiple of the record length keeps every s-th frame without a copy.
 * defs_h is a HOST array of n_defs records of six int32 [kind, a0, a1, a2, a3, out_column]:
 *   DCV_FEAT_DISTANCE        out[col]     = |p1 - p0|                      (a2, a3 ignored)
 *   DCV_FEAT_TORSION_SINCOS  out[col]     = sin, out[col + 1] = cos of the torsion a0-a1-a2-a3
 *   DCV_FEAT_TORSION         out[col]     = the torsion in radians, (-pi, pi]
 * Arithmetic in float64 on p = (double)x * unit (unit 0.1: Angstrom -> nm), no fused multiply-adds, one rounding to
 * float32 on store.  Distance: sqrt of the three squares added in x, y, z order.  Torsion: b0 = p1-p0, b1 = p2-p1,
 * b2 = p3-p2, n1 = b0 x b1, n2 = b1 x b2, x = n1.n2, y = ((n1 x n2).b1)/|b1| (0 when |b1| = 0); angle = atan2(y, x),
 * sin = y/r, cos = x/r with r = hypot(x, y), and (0, 1) when r = 0 (collinear or coincident atoms).  Periodic
 * boundaries are NOT applied.  Non-finite coordinates propagate to the output.
 * Every record is validated before anything is launched: an atom index outside [0, n_atoms), an output column that
 * does not fit ldo or an unknown kind is DCV_EINVAL; so is a set of used atoms of which one frame does not fit LDS
 * (5461 atoms), or, with n_frames > 0, a layout whose last element -- (n_frames - 1) frame_stride + (n_atoms - 1)
 * atom_stride + 2 comp_stride -- overflows or does not lie below 2^60 ("do not fit the address space"; so for every
 * entry that takes these strides).  The records are copied into the workspace; one that is too small is DCV_ENOMEM,
 * nothing launched.
 * A workgroup owns 16 frames (fewer when 16 frames of the staged atoms exceed 48 KB of LDS).  Staged per frame: the
 * index range [min, max] of the atoms the records name when the innermost stride is 1 and they fill at least half of
 * it, otherwise exactly the named atoms.  Algorithmic traffic per frame: 12 bytes per staged atom + 4 per output column. */
#define DCV_FEAT_DISTANCE 0
#define DCV_FEAT_TORSION_SINCOS 1
#define DCV_FEAT_TORSION 2
size_t dcv_featurize_workspace(int64_t n_frames, int32_t n_atoms, int32_t n_defs);
int dcv_featurize(const float* xyz_d, int64_t n_frames, int64_t frame_stride, int64_t atom_stride, int64_t comp_stride,
                  int32_t n_atoms, const int32_t* defs_h, int32_t n_defs, double unit,
                  float* out_d, int64_t ldo, void* ws_d, size_t ws_bytes, void* stream);

/* ---- featurise and project in one launch (project_trajectory) ------------------------------------------------------
 * dcv_featurize followed by dcv_project_linear without the frames x features matrix: coordinates in (addressed as in
 * dcv_featurize), n_frames x d collective variables out, d <= 16.  Replaces, for a linear CV, what the reference hands
 * to PLUMED through write_plumed_files (DISTANCE / TORSION commands and COMBINE lines evaluated during a simulation).
 * rec_h is a HOST array of n_rec records of eight int32 [kind, a0, a1, a2, a3, feature0, feature1, 0]: kind and atoms as
 * in dcv_featurize; feature0 is the feature index (row of W, entry of fmean / frange) of the record's value -- the sine
 * of a DCV_FEAT_TORSION_SINCOS record, whose cosine is feature1.  An index of -1 means the value is not a feature (a
 * sine or a cosine whose partner the model dropped); the single-valued kinds have feature1 = -1.
 * Per frame and output column j:
 *   f_i   the value dcv_featurize would store for feature i: float64 arithmetic, rounded once to float32;
 *   xn_i  = (f_i - fmean_i) / frange_i in float32 IEEE, the bits dcv_normalize forms (f_i when both vectors are NULL);
 *   y_j   = sum_i (double)xn_i * (double)W[i][j], accumulated in float64;
 *   out_j = (float)((y_j + bias_j - cvmean_j) / cvrange_j), evaluated in float64 and rounded once
 * (bias_d NULL = 0; cvmean_d / cvrange_d NULL = 0 / 1, both or neither).  The order of the sum over i is a function of
 * the record list and d alone, so a frame's result depends on nothing but its own coordinates: it is bit-identical for
 * any frame count, chunking of the frames between calls and layout of the coordinates.  out_d has row stride ldo >= d;
 * minmax_d (2*d float32: per-column min then max of the stored values, or NULL) is reduced per workgroup and folded by
 * the finishing launch of dcv_project_linear, without floating-point atomics.
 * Validated before anything is launched (DCV_EINVAL): kinds, atom indices, feature indices in [-1, F) with at least one
 * >= 0 per record, every feature in [0, F) written by exactly one record, 1 <= d <= 16, ldo >= d, fmean / frange both or
 * neither, the strides, one frame of the staged atoms within LDS (5461 atoms); a workspace that is too small is
 * DCV_ENOMEM; then, with n_frames > 0, a layout that does not fit the address space (DCV_EINVAL, as in dcv_featurize).
 * n_frames = 0 is DCV_OK.  Algorithmic traffic per frame: 12 bytes per staged atom + 4*d. */
size_t dcv_featurize_project_workspace(int64_t n_frames, int32_t n_atoms, int32_t n_rec, int32_t F, int32_t d);
int dcv_featurize_project(const float* xyz_d, int64_t n_frames, int64_t frame_stride, int64_t atom_stride, int64_t comp_stride,
                          int32_t n_atoms, const int32_t* rec_h, int32_t n_rec, int32_t F, double unit,
                          const float* fmean_d, const float* frange_d, const float* W_d, int32_t d,
                          const float* bias_d, const float* cvmean_d, const float* cvrange_d,
                          float* out_d, int64_t ldo, float* minmax_d, void* ws_d, size_t ws_bytes, void* stream);

/* ---- optimal rigid superposition (analyze_geometry: RMSD, average structure, RMSF) --------------------------------
 * Fits every frame onto a reference structure on the n_fit atoms fit_h (weights fit_w_h, NULL = all 1) and measures
 * on the n_sel atoms sel_h.  Coordinates are addressed as in dcv_featurize (xyz_d, the three strides, n_atoms); no
 * unit conversion: Angstrom in, Angstrom out.  Row-vector convention.  Per frame, with c_mob and c_ref the weighted
 * centroids of the frame's fit atoms and of fit_ref_h (n_fit x 3), R is the PROPER rotation (det = +1) that minimises
 * sum_i w_i |(x_i - c_mob) . R - (y_i - c_ref)|^2 and aligned = (x - c_mob) . R + c_ref.  Outputs, each may be NULL:
 *   transform_d  n x 16   R row-major (9), c_mob (3), c_ref (3), fit RMSD sqrt(sum_i w_i |residual_i|^2 / sum_i w_i)
 *   rmsd_d       n x 2    fit RMSD, then the unweighted sqrt(mean over sel |aligned - sel_ref|^2); the second entry is
 *                         0 when sel_ref_h (n_sel x 3) is NULL
 *   aligned_d    n x lda  the selected atoms of every frame (x, y, z of atom 0, of atom 1, ...), rounded once to
 *                         float32; lda >= 3 n_sel
 *   moments_d    n_sel x 3 x 2   per selected atom and component the sum over the frames of d and of d^2, with
 *                         d = aligned - sel_ref (the shift keeps the sums free of cancellation); needs sel_ref_h
 * Arithmetic: float64 behind the float32 load.  The coordinates are centred before the 3 x 3 correlation is formed;
 * the rotation is the eigenvector of the largest eigenvalue of Horn's symmetric 4 x 4 quaternion matrix, found by
 * cyclic Jacobi rotations (convergence test, at most 16 sweeps); both RMSDs come from the residuals of the
 * transformed coordinates.  A mirror image of the reference comes back with the (larger) RMSD of the best proper
 * rotation.  One or two fit atoms, collinear and coplanar sets are legal: the RMSD is unique where R is not, and R is
 * a rotation in every case.  Non-finite coordinates propagate to the outputs of their frame.
 * One launch stages the union of the fit and the selected atoms of 16 frames per workgroup into LDS as dcv_featurize
 * does (fewer frames when 48 KB would be exceeded) and reads them from there only; at most DCV_SUPERPOSE_MAX_GROUPS
 * workgroups stride over the tiles.  The moments are kept as float64 partials per workgroup in LDS (48 bytes per
 * selected atom), written once and added in workgroup order by a second small launch: no floating-point atomics,
 * bit-identical from run to run.
 * Everything is validated before anything is launched.  DCV_EINVAL: an index outside [0, n_atoms); n_fit < 1; a
 * weight that is negative or not finite, or weights that do not sum to a positive number; lda < 3 n_sel; moments
 * without sel_ref_h; bad strides; one frame of the staged atoms above 64 KB of LDS (5461 atoms), or that frame plus
 * the parked transform (96 bytes, with aligned_d or moments_d) and the moment partials above 64 KB; with n_frames > 0
 * and behind every other refusal, a layout that does not fit the address space (as in dcv_featurize).  DCV_ENOMEM: a
 * workspace that is too small.  n_frames = 0 is DCV_OK.  The reference and both atom lists are copied into the
 * workspace.  Algorithmic traffic per frame: 12 bytes per staged atom, plus 12 per selected atom with aligned_d. */
#define DCV_SUPERPOSE_MAX_GROUPS 768   /* upper bound of workgroups (and of moment partials) of one call */
size_t dcv_superpose_workspace(int64_t n_frames, int32_t n_atoms, int32_t n_fit, int32_t n_sel);
int dcv_superpose(const float* xyz_d, int64_t n_frames, int64_t frame_stride, int64_t atom_stride, int64_t comp_stride,
                  int32_t n_atoms, const int32_t* fit_h, const double* fit_w_h, const double* fit_ref_h, int32_t n_fit,
                  const int32_t* sel_h, const double* sel_ref_h, int32_t n_sel, double* transform_d, double* rmsd_d,
                  float* aligned_d, int64_t lda, double* moments_d, void* ws_d, size_t ws_bytes, void* stream);

/* ---- frame interpolation (traj_augmentation) -----------------------------------------------------------------------
 * Replaces scipy.interpolate.PchipInterpolator / Akima1DInterpolator(method='makima') along the frame axis of the
 * (frames, atoms, 3) array in interpolate_trajectory, modules/md/md.py:1091-1121.  The n_knots frames of xyz_d are the
 * knots, addressed as in dcv_featurize (the three strides, n_atoms; dense rows or DCD frame records in place, a frame
 * stride that is a multiple of the record length); knot k sits at time k.  t_h is a HOST array of n_out query times,
 * finite and non-decreasing (copied into the workspace).  sel_h is a HOST array of the n_sel atoms to emit, in output
 * order; NULL = all n_atoms atoms (n_sel is then ignored).  noise_d, optional, holds n_out x n_sel x 3 float64, dense,
 * in (frame, atom, xyz) order.  Coordinate c of selected atom s of output frame j goes to
 * out_d[j*out_frame_stride + s*out_atom_stride + c*out_comp_stride] (strides in ELEMENTS, all >= 1): a dense
 * (n_out, n_sel, 3) array, or the X / Y / Z planes of DCD frame records.  Only those elements are written.
 * Arithmetic: float64 behind the float32 load, no fused multiply-adds, out = (float)(p(t) + noise), rounded once.
 * With y a column, m_k = y[k+1] - y[k] (exact in float64), K = clamp(floor(t), 0, n_knots - 2) and s = t - K:
 *   piece (both kinds: scipy's CubicHermiteSpline -> PPoly with h = 1)  T = d_K + d_{K+1} - 2 m_K,
 *     p = y_K + d_K s + (m_K - d_K - T) s^2 + T s^3.  t outside [0, n_knots - 1] uses the end piece when
 *     extrapolate != 0 and is NaN when extrapolate == 0.  A finite result at t == k is y_k exactly.
 *   DCV_INTERP_PCHIP derivatives (scipy PchipInterpolator._find_derivatives, h = 1)
 *     interior  d_k = 0 when sign(m_{k-1}) != sign(m_k) or either is 0, otherwise 1 / ((3/m_{k-1} + 3/m_k) / 6);
 *     ends      with m0 the end slope and m1 its neighbour e = (3 m0 - m1) / 2; e = 0 when sign(e) != sign(m0);
 *               otherwise e = 3 m0 when sign(m0) != sign(m1) and |e| > 3 |m0|; otherwise e is kept;
 *     n_knots == 2: both derivatives are m_0.
 *   DCV_INTERP_MAKIMA derivatives (scipy 1.15 Akima1DInterpolator, method='makima'); n_knots >= 3 (scipy's own result
 *     for two knots reads an uninitialised slope).  With M the padded slopes: M[2:-2] = m, M[1] = 2M[2] - M[3], then
 *     M[0] = 2M[1] - M[2], M[-2] = 2M[-3] - M[-4], then M[-1] = 2M[-2] - M[-3]:
 *       f1_k = |M[k+3] - M[k+2]| + |M[k+3] + M[k+2]| / 2,   f2_k = |M[k+1] - M[k]| + |M[k+1] + M[k]| / 2,
 *       d_k = (f1_k M[k+1] + f2_k M[k+2]) / (f1_k + f2_k) where f1_k + f2_k > 1e-9 G, (M[k+3] + M[k]) / 2 elsewhere.
 *     G is the maximum of f1 + f2 over EVERY knot of EVERY selected column (scipy takes one maximum over the whole
 *     array: one atom of large amplitude switches quiet atoms to the plain average).  A pass over the knots writes one
 *     partial maximum per wave with plain stores, a one-workgroup launch reduces them, the evaluation reads the
 *     result: no atomics, and a maximum does not depend on the order, so the output is bit-identical from run to run.
 *     Non-finite values are left out of G.
 * A non-finite input coordinate spoils its own column only.
 * Everything is validated before anything is launched.  DCV_EINVAL: an unknown kind; n_knots < 2 (< 3 for makima); a
 * selection index outside [0, n_atoms); n_sel < 1 with a selection; bad strides; a decreasing or non-finite time; with
 * n_out > 0 and behind every other refusal, an input layout (n_knots frames of n_atoms atoms) or an output layout (n_out
 * frames of n_sel atoms) that does not fit the address space (as in dcv_featurize).
 * DCV_ENOMEM: a workspace that is too small.  n_out = 0 is DCV_OK.
 * A wave owns 64 adjacent coordinate columns and a run of at least 64 consecutive output frames; a lane walks its run
 * in ascending t with the six knots around floor(t) and the following one in registers and loads one knot whenever
 * floor(t) advances.  Nothing is staged in LDS: no limit on the number of atoms.  Algorithmic traffic per output frame:
 * 12 bytes per selected atom written, plus 24 read with noise_d; reading the knots once costs 12 bytes per knot and
 * selected atom (once more for makima's G). */
#define DCV_INTERP_PCHIP 0
#define DCV_INTERP_MAKIMA 1
size_t dcv_interpolate_workspace(int64_t n_knots, int32_t n_atoms, int32_t n_sel, int64_t n_out);
int dcv_interpolate(const float* xyz_d, int64_t n_knots, int64_t frame_stride, int64_t atom_stride, int64_t comp_stride,
                    int32_t n_atoms, const int32_t* sel_h, int32_t n_sel, int32_t kind, int32_t extrapolate,
                    const double* t_h, int64_t n_out, const double* noise_d,
                    float* out_d, int64_t out_frame_stride, int64_t out_atom_stride, int64_t out_comp_stride,
                    void* ws_d, size_t ws_bytes, void* stream);

/* ---- rigid transform of whole frames (align_trajectories) ----------------------------------------------------------
 * Applies to EVERY atom of frame f the transform in row f of transform_d: the first 15 doubles of a row of
 * dcv_superpose's transform output -- R row-major (row-vector convention), c_mob, c_ref --, rows ldt >= 15 doubles
 * apart, so the n x 16 tensor is passed as it is.  For every frame f, atom a and component c = 0, 1, 2:
 *     p   = (double)x[f, a, :] - c_mob[f]
 *     out = (float)(p0 R[f][0][c] + p1 R[f][1][c] + p2 R[f][2][c] + c_ref[f][c])
 * summed left to right in float64 without fused multiply-adds; the store is the one rounding.  No unit conversion.
 * The input is addressed as in dcv_featurize (xyz_d, the three strides in elements: dense rows, DCD frame records in
 * place with or without the unit-cell block, a frame stride that skips frames); coordinate c of atom a of frame f goes
 * to out_d[f*out_frame_stride + a*out_atom_stride + c*out_comp_stride] (strides >= 1) as in dcv_interpolate: a dense
 * (n, A, 3) array or the planes of a DCD record image.  Only those elements are written.  Nothing is staged in LDS:
 * there is no limit on the number of atoms (dcv_superpose's `aligned` output stops at 5461).  A non-finite transform
 * row gives non-finite coordinates in its own frame only.
 * Everything is validated before anything is launched.  DCV_EINVAL: a NULL pointer or one off the 4-byte (transform:
 * 8-byte) grid; n_atoms <= 0; n_frames < 0; bad strides (input: frame < 0, atom or component < 1; output: any < 1);
 * ldt < 15; an input element range [xyz_d, xyz_d + last] that overlaps the output's, both computed from the strides
 * (the map is not in place), or transform rows that overlap the output.  n_frames = 0 is DCV_OK and launches nothing.  No workspace.
 * One launch; a thread owns four consecutive atoms of one frame (16-byte accesses where the atom stride is 1 or the
 * rows are dense; the first and the last group of a row are moved inside the row and overlap their neighbours, whose
 * atoms are then stored twice with the same bits), several frames share a workgroup when there are few atoms, at most
 * 2048 workgroups stride over the rest.  Algorithmic traffic: 12 bytes read and 12 written per atom and frame, 120 per frame for the transform. */
int dcv_transform_frames(const float* xyz_d, int64_t n_frames, int64_t frame_stride, int64_t atom_stride, int64_t comp_stride,
                         int32_t n_atoms, const double* transform_d, int64_t ldt,
                         float* out_d, int64_t out_frame_stride, int64_t out_atom_stride, int64_t out_comp_stride, void* stream);

/* ---- GROMACS XTC frames decoded on the device (import_trajectories) ---------------------------------------------------
 * bytes_d holds the bytes of an XTC file, or a contiguous slice of them that starts on a multiple of 4 bytes of the file,
 * 4-byte aligned; frames_h, on the host, one descriptor per frame to decode (trajectory.index_xtc makes them; choosing
 * descriptors is how a frame stride or a sub-range is applied).  Coordinate c of atom a of decoded frame f goes to
 * out_d[f*out_frame_stride + a*out_atom_stride + c*out_comp_stride] (strides in ELEMENTS, all >= 1) as in
 * dcv_interpolate and dcv_transform_frames: a dense (n, A, 3) array or the planes of a DCD record image.  Only those
 * elements are written.  status_d[f] = 0: the frame decoded; anything else: its stream was inconsistent
 * (DCV_XTC_*) and the coordinates of the frame from the first inconsistency on are left unwritten.
 *
 * The file (magic 1995; every integer and float big-endian).  A frame is
 *     int32 magic (1995)  int32 natoms  int32 step  float32 time  float32 box[9]  int32 natoms
 *     natoms <= 9 :  3*natoms float32 (nm), nothing else                                        (descriptor: raw != 0)
 *     natoms >  9 :  float32 precision  int32 minint[3]  int32 maxint[3]  int32 smallidx  int32 nbytes
 *                    nbytes of payload, padded with zeros to a multiple of 4
 * and `offset` of a descriptor is the byte offset, inside bytes_d, of the payload (of the floats for a raw frame).
 * The payload is a bit stream, most significant bit first.  With FIRSTIDX = 9 and
 *   magic[] = 0 x9, 8,10,12,16,20,25,32,40,50,64,80,101,128,161,203,256,322,406,512,645,812,1024,1290,1625,2048,2580,
 *     3250,4096,5060,6501,8192,10321,13003,16384,20642,26007,32768,41285,52015,65536,82570,104031,131072,165140,208063,
 *     262144,330280,416127,524287,660561,832255,1048576,1321122,1664510,2097152,2642245,3329021,4194304,5284491,6658042,
 *     8388607,10568983,13316085,16777216                                                   (73 entries, indices 0..72)
 *   sizeint[k] = maxint[k] - minint[k] + 1
 *   if any sizeint > 0xffffff: bitsizeint[k] = smallest b with 2^b > sizeint[k], at most 32;  bitsize = 0
 *   else: bitsize = bit length of the product sizeint[0]*sizeint[1]*sizeint[2]                        (up to 72 bits)
 *   smaller = magic[max(FIRSTIDX, smallidx-1)]/2;  smallnum = magic[smallidx]/2;  sizesmall = magic[smallidx];  run = 0;  i = 0
 *   while i < natoms:
 *       this = bitsize == 0 ? three fields of bitsizeint[k] bits : unpack3(bitsize, sizeint);   i++;   this += minint;   prev = this
 *       flag = 1 bit;  is_smaller = 0
 *       if flag: run = 5 bits;  is_smaller = run % 3;  run -= is_smaller;  is_smaller -= 1    (run otherwise KEEPS its last value)
 *       if run > 0:
 *           for k = 0, 3, ..., < run:
 *               this = unpack3(smallidx, {sizesmall x3});  i++;  this += prev - smallnum
 *               if k == 0: swap(this, prev); emit(prev)       (the water swap: the second atom of a run is written first)
 *               else:      prev = this
 *               emit(this)
 *       else: emit(this)
 *       smallidx += is_smaller
 *       if is_smaller < 0: smallnum = smaller;  smaller = smallidx > FIRSTIDX ? magic[smallidx-1]/2 : 0
 *       if is_smaller > 0: smaller = smallnum;  smallnum = magic[smallidx]/2
 *       sizesmall = magic[smallidx]
 *   unpack3(nbits, sizes): read nbits/8 whole bytes, LEAST significant byte first, then the nbits%8 remaining bits as the
 *       top byte, into one unsigned integer v;  n2 = v % sizes[2]; v /= sizes[2];  n1 = v % sizes[1];  n0 = v / sizes[1]
 *       (v is held in three 32-bit limbs and divided limb by limb; n0 is the low 32 bits of the last quotient).
 * emit(i) writes x = (float)i * inv with inv = 1.0f / precision, then x * scale (scale = 10 for Angstrom): two float32
 * multiplications, never contracted -- what xdrfile followed by a unit conversion in float32 produce.  A raw frame
 * writes value * scale.  Integer sums wrap in 32 bits.
 *
 * A lane owns a frame (inside a frame the stream is strictly sequential); the bit reader keeps a 64-bit window refilled
 * by 4-byte loads with a byte swap; every iteration decodes one atom in every lane, so the lanes of a wave stay within one
 * atom of each other, a lane stages its last nine atoms in LDS and the wave stores blocks of eight atoms of its 64 frames
 * in contiguous pieces (96 bytes for dense rows, 32 for planes).  No stream, however corrupt, reads or writes out of range: the reader returns zero bits behind nbytes and marks the frame (DCV_XTC_SHORT); the atom
 * counter is checked before every emit and a run that would pass natoms marks the frame and stops (DCV_XTC_RUN); a
 * smallidx that leaves [9, 72] marks the frame and stops (DCV_XTC_SMALLIDX); maxint < minint, or a precision that is not
 * finite and positive, mark it before anything is read (DCV_XTC_HEADER).
 * Validated on the host before anything is launched (DCV_EINVAL): NULL pointers; n_atoms < 1; n_frames < 0; bytes_d or
 * out_d off the 4-byte grid; a descriptor whose offset is negative or no multiple of 4, whose nbytes is negative, or whose
 * bytes (nbytes rounded up to 4; 12*n_atoms for a raw frame) end behind n_bytes; a raw flag that disagrees with
 * n_atoms <= 9; output strides below 1; an output, status or workspace range that overlaps the input bytes or each other's.
 * The descriptors are copied into the workspace; one that is too small is DCV_ENOMEM, nothing launched.  n_frames = 0 is
 * DCV_OK.  Algorithmic traffic per frame: its payload read once, 12 bytes per atom written. */
#define DCV_XTC_OK 0
#define DCV_XTC_SHORT 1     /* the stream needed bits behind nbytes */
#define DCV_XTC_RUN 2       /* a run of small atoms would pass natoms */
#define DCV_XTC_SMALLIDX 3  /* smallidx left [9, 72] */
#define DCV_XTC_HEADER 4    /* maxint < minint or a precision that is not finite and positive */
typedef struct dcv_xtc_frame {
    int64_t offset;      /* bytes from bytes_d to the payload (raw: to the floats); a multiple of 4 */
    int32_t nbytes;      /* payload bytes (raw: ignored) */
    int32_t smallidx;
    float precision;
    int32_t raw;         /* != 0: 3*n_atoms big-endian float32, no payload (n_atoms <= 9) */
    int32_t minint[3];
    int32_t maxint[3];
} dcv_xtc_frame;
size_t dcv_xtc_decode_workspace(int64_t n_frames);
int dcv_xtc_decode(const void* bytes_d, int64_t n_bytes, const dcv_xtc_frame* frames_h, int64_t n_frames, int32_t n_atoms,
                   float scale, float* out_d, int64_t out_frame_stride, int64_t out_atom_stride, int64_t out_comp_stride,
                   int32_t* status_d, void* ws_d, size_t ws_bytes, void* stream);

/* ---- GROMACS XTC frames encoded on the device (traj_cluster: the frames of every cluster) ---------------------------
 * The inverse of dcv_xtc_decode, in two launches.  dcv_xtc_encode compresses frames into *slots*, one per frame, because
 * the length of a frame's stream is known only when it has been written; the host sums the lengths; dcv_xtc_pack writes
 * the finished big-endian frames -- header, fields, payload, zero padding -- into one contiguous file image.
 *
 * Input.  Coordinate c of atom a of source frame s is xyz_d[s*frame_stride + a*atom_stride + c*comp_stride] (strides in
 * ELEMENTS, all >= 1), as in dcv_featurize: dense rows or the planes of DCD frame records, read in place.  frames_h (HOST,
 * or NULL) holds n_frames indices into the n_src_frames source frames, in any order, repeats allowed: output frame f is
 * source frame frames_h[f].  NULL: output frame f is source frame f, n_frames <= n_src_frames.  The indices are checked
 * and copied into the workspace; gathering costs no pass of its own.
 *
 * Quantisation, per coordinate, in float32 and never contracted into a fused multiply-add:
 *     lf = (x * inv_scale) * precision          (x in Angstrom: inv_scale = 0.1f;  the usual precision is 1000)
 *     i  = (int32)truncf(lf + copysignf(0.5f, lf))
 * A frame with a coordinate that is not finite is marked DCV_XTC_ENC_NONFINITE; otherwise one with a value for which
 * !(fabsf(lf) < 2147483520.0f) -- the largest float32 below 2^31 -- is marked DCV_XTC_ENC_RANGE.  Nothing is written to
 * the slot of a marked frame and its descriptor keeps offset, precision and raw only.  Quantising what dcv_xtc_decode
 * wrote (scale 10) gives back the integers of the file: a trajectory that came from an .xtc is re-encoded losslessly.
 *
 * The frame.  minint / maxint per component over the frame; sizeint, bitsize or the three bitsizeint, the payload's bit
 * order and unpack3 as described for dcv_xtc_decode above; pack3 is the inverse of unpack3: v = (n0*sizes[1] + n1)*sizes[2]
 * + n2 in three 32-bit limbs, nbits/8 whole bytes LEAST significant first, then the nbits%8 remaining bits.  natoms <= 9 is
 * the raw form: 3*natoms big-endian float32 of x * inv_scale (marked only for coordinates that are not finite).
 *
 * The policy -- which legal stream is written.  q[a] the quantised atoms, N = natoms, all differences exact (64 bits):
 *   starting smallidx:  mindiff = min over a >= 1 of |dx| + |dy| + |dz| between q[a] and q[a-1];
 *                       s = 9;  while s < 72 and magic[s] < mindiff: s++
 *   the group that starts at atom p with the current s:   smallnum = magic[s]/2;  sizesmall = magic[s]
 *       reach(a, b): 0 <= a_c - b_c + smallnum < sizesmall for all three components
 *       r = 0;  if p+1 < N and reach(q[p], q[p+1]):  r = 1, prev = q[p]      (the water swap: q[p+1] is written as the
 *                                                                             full-range atom, q[p] is coded against it)
 *           while r < 8 and p+1+r < N and reach(q[p+1+r], prev):  prev = q[p+1+r];  r++
 *       (a run always begins with the swap: without it the group is the single atom p.)  The group covers atoms p .. p+r.
 *   step of smallidx:   r == 0:  +1 when s < 72, else 0
 *                       r >  0:  -1 when s > 9 and every component of every difference coded in the group has
 *                                |d| < magic[max(9, s-1)]/2, else 0
 *   flag = 0 (the run value is reused) exactly when 3r equals the run value written last (0 at the start of a frame) and
 *   the step is 0; otherwise flag = 1 and the 5-bit value 3r + step + 1.
 * tests/xtc_encode_oracle.py restates all of it in Python; the device bytes are compared with it bit for bit.
 *
 * Capacity.  A frame needs at most 102*natoms bits: 96 for a full-range atom plus 6 of flag and run value, and a small
 * atom costs smallidx <= 72 bits.  The slot of frame f is dcv_xtc_encode_slot_bytes(natoms) = ceil(102*natoms/8) rounded
 * up to 4 bytes, at slots_d + f*slot; it receives the payload and its zero padding to a multiple of 4 (a raw frame: the
 * floats) and nothing behind that; the writer checks the slot's end before every store all the same.
 * desc_d[f] (DEVICE) is the dcv_xtc_frame of frame f -- offset = f*slot, nbytes, smallidx, precision, raw, minint, maxint;
 * a raw frame has zeros in all of them but offset and raw, as trajectory.index_xtc reports it -- and status_d[f] its status.
 *
 * A lane owns a frame, one-wave workgroups, one atom consumed per iteration in every lane; the wave stages blocks of 16
 * atoms of its 64 frames in LDS with loads that are contiguous along the atoms of a frame (two blocks resident: the policy
 * looks at most 8 atoms ahead); two passes over the atoms (minima, maxima and mindiff; then the stream), quantising from
 * the staged floats both times; a 64-bit window, finished 32-bit words stored byte-swapped.  No atomics.
 * Validated on the host before anything is launched (DCV_EINVAL): NULL pointers; n_atoms < 1; negative frame counts;
 * misaligned pointers (4 bytes; descriptors and workspace 8); strides below 1; an index outside [0, n_src_frames);
 * n_frames > n_src_frames without indices; a precision that is not finite and positive; coordinates, slots, descriptors,
 * status words and workspace that overlap.  DCV_ENOMEM: a workspace below dcv_xtc_encode_workspace(n_frames) when indices
 * are given, or slots_bytes below n_frames slots.  Nothing is launched or written then.  n_frames = 0 is DCV_OK.
 * Algorithmic traffic per frame: 12 bytes per atom read twice (the second time from L2 at best), its payload written.
 *
 * dcv_xtc_pack.  desc_h: the descriptors as dcv_xtc_encode left them, downloaded (HOST); image_offset_h[f]: where frame f
 * begins in the image -- the prefix sum over 56 + 36 + nbytes rounded up to 4, or 56 + 12*natoms for raw frames -- or a
 * negative value for a frame that is not packed (a marked one); step_h, time_h and box_h (9 floats a frame; NULL: zeros)
 * fill the header.  A wave copies a frame in 4-byte words.  DCV_EINVAL: NULL or misaligned pointers; a descriptor whose
 * raw flag disagrees with n_atoms, whose nbytes is negative or above the slot size, or whose payload does not lie on the
 * 4-byte grid inside slots_bytes; an image offset off the 4-byte grid, below the end of the frame before or whose frame ends
 * behind image_bytes; slots, image and workspace that overlap.  DCV_ENOMEM: a workspace below
 * dcv_xtc_pack_workspace(n_frames).  Traffic: every packed frame's bytes read once and written once. */
#define DCV_XTC_ENC_NONFINITE 1   /* a coordinate of the frame is NaN or infinite */
#define DCV_XTC_ENC_RANGE 2       /* a coordinate of the frame does not fit a 32-bit integer at this precision */
size_t dcv_xtc_encode_slot_bytes(int32_t n_atoms);
size_t dcv_xtc_encode_workspace(int64_t n_frames);
int dcv_xtc_encode(const float* xyz_d, int64_t n_src_frames, int64_t frame_stride, int64_t atom_stride, int64_t comp_stride,
                   int32_t n_atoms, const int64_t* frames_h, int64_t n_frames, float inv_scale, float precision,
                   void* slots_d, size_t slots_bytes, dcv_xtc_frame* desc_d, int32_t* status_d, void* ws_d, size_t ws_bytes,
                   void* stream);
size_t dcv_xtc_pack_workspace(int64_t n_frames);
int dcv_xtc_pack(const void* slots_d, size_t slots_bytes, const dcv_xtc_frame* desc_h, const int64_t* image_offset_h,
                 const int32_t* step_h, const float* time_h, const float* box_h, int64_t n_frames, int32_t n_atoms,
                 void* image_d, size_t image_bytes, void* ws_d, size_t ws_bytes, void* stream);

/* ---------------------------------------------------------------- normalisation (a3)
 * Replaces LinearCalculator.normalize_data, cv_calculator.py:833-835
 * (data.sub_(mean).div_(range) in float32).  Y may alias X (in place, as the reference). */
int dcv_normalize(const float* X_d, float* Y_d, int64_t n, int32_t F, int64_t ldx, int64_t ldy,
                  const float* mean_d, const float* range_d, void* stream);

/* ---------------------------------------------------------------- lagged covariance (a4-a7)
 * Replaces create_timelagged_dataset + the two torch.einsum("ij,ik,i->jk") of
 * mlcolvar.core.stats.TICA.compute (call sites cv_calculator.py:2247-2261, 2309-2378) and the
 * X^T X of sklearn PCA (cv_calculator.py:2204-2207).
 * Pairs are (i, i+lag), i = 0 .. n_pairs-1; rows 0 .. n_pairs+lag-1 of X must be readable
 * (the last `lag` rows are the halo a shard borrows from its successor).  With
 * z = x - shift (shift_d may be NULL = 0), out_d receives 2F + 2F*F float64:
 *   [ a = sum z_t | b = sum z_lag | A = sum z_t z_t^T | B = sum z_t z_lag^T ]   (raw sums).
 * All four blocks combine over shards by addition.  lag = 0 computes only a and A (PCA);
 * B and b are then zero.  FP32 MFMA (v_mfma_f32_32x32x2_f32), fp32 accumulation over chunks
 * of <= 2048 rows, chunk partials summed in float64 in a fixed order (deterministic).  With a shift the column sums a, b come
 * from the kernel's own fragments, accumulated in float32 inside a chunk: shift_d must then be (close to) the column
 * means -- what the calculators pass -- for those sums to keep float64-grade accuracy; without a shift a separate float64
 * statistics pass forms them.
 * Algorithmic work: 4*n_pairs*F^2 flop (2*n*F^2 for lag 0), 4*n*F bytes. */
size_t dcv_lagged_cov_workspace(int64_t n_pairs, int32_t F, int32_t lag);
int dcv_lagged_cov(const float* X_d, int64_t n_pairs, int32_t F, int64_t ld, int32_t lag,
                   const float* shift_d, double* out_d, void* ws_d, size_t ws_bytes, void* stream);

/* ---------------------------------------------------------------- linear projection (a13, a14)
 * Replaces LinearCalculator.project_data / normalize_cv, cv_calculator.py:918-991:
 *   p = ((x - fmean)/frange) @ W ; out = (p - cvmean)/cvrange.
 * fmean_d/frange_d NULL => input already normalised; cvmean_d/cvrange_d NULL => raw p.
 * bias_d (d floats or NULL) is added to p before the CV normalisation.
 * W is F x d row-major (the layout of cv_weights.npy), d <= 16.
 * minmax_d (2*d float32: per-column min then max of `out`, or NULL) combines over shards by
 * min/max.  out_d may be NULL when only the extrema are wanted.  HBM-bound:
 * 4*F + 4*d bytes per frame. */
size_t dcv_project_linear_workspace(int64_t n, int32_t F, int32_t d);
int dcv_project_linear(const float* X_d, int64_t n, int32_t F, int64_t ld,
                       const float* fmean_d, const float* frange_d, const float* W_d, int32_t d,
                       const float* bias_d, const float* cvmean_d, const float* cvrange_d,
                       float* out_d, float* minmax_d, void* ws_d, size_t ws_bytes, void* stream);

/* ---------------------------------------------------------------- MLP engine (a8-a12, a15)
 * Replaces mlcolvar.cvs.DeepTICA / AutoEncoderCV + the lightning training loop driven by
 * NonLinear.train, cv_calculator.py:1456-1553 (models :2471-2492, :2569-2590), and the
 * whole-tensor forward of NonLinear.project_data / normalize_cv (:1735-1754, :1842-1891).
 *
 * A model is a chain of Linear layers over PRE-NORMALISED input (dcv_normalize applies
 * norm_in once; (x-mean)/range is elementwise, so the result is bit-identical to applying it
 * inside the model).  Parameters live in one flat float32 device buffer, layer by layer,
 * weight (out x in, row-major, torch.nn.Linear layout) then bias (out).
 */
#define DCV_ACT_NONE 0
#define DCV_ACT_LEAKY_RELU 1 /* slope 0.01 */
#define DCV_ACT_RELU 2
#define DCV_ACT_TANH 3
#define DCV_ACT_ELU 4
#define DCV_ACT_SOFTPLUS 5
#define DCV_ACT_SHIFTED_SOFTPLUS 6 /* mlcolvar Shifted_Softplus: softplus(z) - softplus(0) */
#define DCV_ACT_CUSTOM_SIGMOID 7   /* mlcolvar Custom_Sigmoid: 1 / (1 + exp(-3 z)); forced on the decoder output for
                                      min_max_range1 features, cv_calculator.py:1193-1198 */
#define DCV_MAX_LAYERS 16

/* torch.optim.<name> as selected by optimizer.name of the training configuration (cv_calculator.py:1377-1380,
 * model.optimizer_name :1511); single-tensor CPU arithmetic of torch 2.x, float32 state. */
#define DCV_OPT_ADAM 0     /* lr, beta1, beta2, eps, weight_decay (L2 into the gradient), amsgrad */
#define DCV_OPT_ADAMW 1    /* decoupled weight decay: p *= 1 - lr * weight_decay */
#define DCV_OPT_SGD 2      /* lr, momentum, dampening, nesterov, weight_decay */
#define DCV_OPT_RMSPROP 3  /* lr, alpha, eps, weight_decay, momentum, centered */
#define DCV_OPT_ADAGRAD 4  /* lr, lr_decay, eps, weight_decay, initial_accumulator_value */
#define DCV_OPT_ADAMAX 5   /* lr, beta1, beta2, eps, weight_decay */
#define DCV_OPT_NADAM 6    /* lr, beta1, beta2, eps, weight_decay, opt_p[0] = momentum_decay, opt_p[1] = decoupled_weight_decay */
#define DCV_OPT_RADAM 7    /* lr, beta1, beta2, eps, weight_decay, opt_p[1] = decoupled_weight_decay */
#define DCV_OPT_ADADELTA 8 /* lr, opt_p[0] = rho, eps, weight_decay */
#define DCV_OPT_ASGD 9     /* lr, opt_p[0] = lambd, opt_p[1] = alpha, opt_p[2] = t0, weight_decay (the averaged copy `ax` is not a model
                              parameter and is not kept) */
#define DCV_OPT_RPROP 10   /* lr, opt_p[0..1] = etas (minus, plus), opt_p[2..3] = step_sizes (min, max) */

#define DCV_MODEL_DEEPTICA 1 /* loss = -sum(eig^2) of the batch TICA of nn(x_t), nn(x_lag) */
#define DCV_MODEL_AE 2       /* loss = mean(((dec(enc(xn)) - xn) * range)^2) */
/* Variational autoencoder (mlcolvar VariationalAutoEncoderCV, reference cv_calculator.py:2629-2780), in the same descriptor:
 * Linear latent_layer - 1 is the two heads concatenated (mean_nn rows, then log_var_nn rows: dims[latent_layer] = 2d
 * columns, no activation / dropout / batch normalisation); Linear latent_layer reads z = mu + exp(lv / 2) * eps (d columns).
 *   loss = reconstruction + beta * kl,  reconstruction = the AE's loss,  kl = mean over the batch of
 *          -0.5 * sum_j (lv - exp(lv) - mu^2 + 1)
 * eps comes from the caller (dcv_mlp_set_noise), beta from dcv_mlp_set_kl_beta.  Log records are
 * [loss | batch | reconstruction | kl], dcv_mlp_stats() holds [SSE | KL sum].  d <= 8.  Not data-parallel: dcv_mlp_dp_step
 * refuses global_batch != batch (DCV_EINVAL).  Networks that fit in LDS take the fused one-launch step (dcv_mlp_last_path 1, the
 * validation pass of dcv_mlp_eval_steps many batches per launch, each with its own eps rows), the others the layer-by-layer path. */
#define DCV_MODEL_VAE 3

typedef struct dcv_mlp_desc {
    int32_t model;                      /* DCV_MODEL_* */
    int32_t n_layers;                   /* number of Linear layers (AE: encoder + decoder) */
    int32_t dims[DCV_MAX_LAYERS + 1];   /* dims[0] = F ... dims[n_layers] */
    int32_t act[DCV_MAX_LAYERS];        /* activation after each Linear */
    int32_t latent_layer;               /* AE: index of the Linear whose output is the CV
                                           (encoder depth); Deep-TICA: n_layers */
    int32_t lag;                        /* Deep-TICA pair offset in rows */
    int32_t max_batch;                  /* largest number of samples (pairs / frames) per step */
    double tica_reg;                    /* Deep-TICA: C0 + reg*I */
    /* optimiser (torch.optim semantics, cv_calculator.py:1377-1380); fields a given optimiser does not have are ignored */
    double lr, beta1, beta2, eps, weight_decay;
    int32_t optimizer;                  /* DCV_OPT_* */
    int32_t amsgrad;                    /* Adam / AdamW */
    int32_t nesterov;                   /* SGD */
    int32_t centered;                   /* RMSprop */
    double momentum, dampening;         /* SGD, RMSprop (momentum) */
    double alpha;                       /* RMSprop smoothing constant */
    double lr_decay, initial_accumulator_value; /* Adagrad */
    double opt_p[4];                    /* further constants of the optimiser, see DCV_OPT_* */
    /* torch.nn.Dropout(p) behind the activation of each Linear (mlcolvar FeedForward order: Linear, activation,
     * dropout), active in training steps only; 0 = none.  Masks come from a counter-based generator keyed by `seed`.
     * p must lie in [0, 1): dcv_mlp_create refuses p >= 1 (and a negative or non-finite p) with DCV_EINVAL -- the kept
     * values are scaled by 1 / (1 - p).
     * The keep bit of element (row, col) of Linear `layer` in training step `step` is Philox-4x32 with 7 rounds on the counter
     * (row, col >> 2, layer, step) (each mod 2^32) under the key (seed & 0xffffffff, (seed >> 32) + 0x9E3779B9 * rank) (rank:
     * dcv_mlp_set_rank): the four output words cover columns 4 (col >> 2) .. + 3, an element is kept iff its word >= thr,
     * thr = p * 2^32 clamped to [1, 2^32 - 1].  tests/dropout_oracle.py restates it independently. */
    float dropout[DCV_MAX_LAYERS];
    uint64_t seed;
    /* torch.nn.BatchNorm1d(dims[l + 1]) behind Linear l (mlcolvar FeedForward order: Linear, activation, dropout, batchnorm);
     * training steps normalise with the batch statistics (Deep-TICA: of each half of the batch separately, x_t first, as the
     * reference's two forward calls do) and update the running statistics, evaluation steps and inference use the running
     * ones.  weight / bias of the layer follow its Linear in the flat parameter buffer (dcv_mlp_param_offset which = 2, 3). */
    int32_t batchnorm[DCV_MAX_LAYERS];
    double bn_eps, bn_momentum;         /* torch defaults 1e-5, 0.1 */
    /* torch.optim's `maximize`: the update uses the negated gradient (every optimiser; dcv_mlp_grads still holds the gradient
     * of the loss).  ABI version 4. */
    int32_t maximize;
} dcv_mlp_desc;

typedef struct dcv_mlp dcv_mlp; /* opaque; owns parameters, optimiser state and workspaces */

int dcv_mlp_create(const dcv_mlp_desc* desc, dcv_mlp** out);
void dcv_mlp_destroy(dcv_mlp* m);
/* Length of the flat parameter buffer.  Every tensor starts on a 16-byte boundary, so the
 * buffer may hold padding: dcv_mlp_param_offset(m, layer, 0) is the offset (in floats) of the
 * weight of Linear `layer`, (.., 1) of its bias. */
int64_t dcv_mlp_num_params(const dcv_mlp* m);
int64_t dcv_mlp_param_offset(const dcv_mlp* m, int32_t layer, int32_t which);
/* Flat parameter / gradient buffers (device, float32, dcv_mlp_num_params elements).  The
 * gradient buffer is what a data-parallel run all-reduces (SUM) between backward and apply. */
float* dcv_mlp_params(dcv_mlp* m);
float* dcv_mlp_grads(dcv_mlp* m);
int dcv_mlp_set_params(dcv_mlp* m, const float* params_h, void* stream);
int dcv_mlp_get_params(dcv_mlp* m, float* params_h, void* stream);
int dcv_mlp_set_lr(dcv_mlp* m, double lr);
/* beta1 (Adam / AdamW) or momentum (SGD / RMSprop): what torch's OneCycleLR / CyclicLR cycle next to the
 * learning rate (cv_calculator.py:1228-1273 -> lr_scheduler). */
int dcv_mlp_set_momentum(dcv_mlp* m, double value);
/* Deep-TICA, contiguous batches (idx_d == NULL, 1 <= lag <= batch): x_lag of sample i is x_t of sample
 * i + lag, so by default the network is evaluated once on the batch + lag rows both halves share
 * (identical outputs, about half the matrix work; the gradient of a shared row is the sum of its two
 * roles).  enable = 0 evaluates the two halves separately (2 * batch rows), as gathered batches always
 * are -- used by the parity tests to check that both forms agree. */
int dcv_mlp_set_row_sharing(dcv_mlp* m, int32_t enable);
/* AE / VAE: per-feature range of norm_in (device copy is made); needed by the loss. */
int dcv_mlp_set_feature_range(dcv_mlp* m, const float* range_h, void* stream);
/* VAE only: weight beta of the KL term in the following steps (the reference's KL annealing sets it per epoch). */
int dcv_mlp_set_kl_beta(dcv_mlp* m, double beta);
/* VAE only: the standard-normal noise of the following steps, a cursor over the caller's device buffer eps_d
 * (rows x d float32, row-major, not copied: it must stay valid while steps run).  Every VAE training or evaluation step
 * (dcv_mlp_forward, *_step, *_steps) takes the next `batch` rows, in call order; a step that would read past row `rows`
 * returns DCV_ESTATE before anything is launched.  The call rewinds the cursor; dcv_mlp_noise_position returns it. */
int dcv_mlp_set_noise(dcv_mlp* m, const float* eps_d, int64_t rows);
int64_t dcv_mlp_noise_position(const dcv_mlp* m);
/* VAE test hook: the sampled latent z of the last forward (rows x d floats, dense, device). */
int dcv_mlp_latent_sample(dcv_mlp* m, int64_t rows, float* out_d, void* stream);

/* One optimisation / evaluation step, split in phases so that a data-parallel caller can
 * all-reduce between them.  Samples of the batch: idx_d != NULL => sample j uses row
 * idx_d[j] (int64, device) else row row0 + j; Deep-TICA also reads row + lag (rows row0 .. row0 +
 * batch + lag - 1 must exist).
 * `global_batch` is the number of samples over ALL ranks (= batch on one GPU).
 *
 *   dcv_mlp_forward   forward pass (train != 0: dropout active, as in model.train(); 0: model.eval());
 *                     train != 0 with batch == 1 while any layer is batch-normalised is REFUSED (DCV_EINVAL, nothing
 *                     launched, no state changed; also through dcv_mlp_train_step / _steps / _dp_step): every forward call
 *                     of the step -- the batch, or each half of a Deep-TICA batch -- would have one row, on which
 *                     torch.nn.BatchNorm1d raises in training mode;
 *                     Deep-TICA: leaves the batch statistics
 *                     [sum f_t (d) | sum f_lag (d) | sum f_t f_t^T (d*d) | sum f_t f_lag^T (d*d)]
 *                     as float64 in dcv_mlp_stats() (all-reduce SUM across ranks);
 *                     AE: leaves [sum of squared errors] there.
 *   dcv_mlp_backward  loss + gradients of this rank's samples -> dcv_mlp_grads()
 *                     (already scaled for the global batch; all-reduce SUM across ranks).
 *                     Appends one record to the metrics log (see dcv_mlp_read_log).
 *                     train = 0: evaluation only (loss logged, no gradients).
 *   dcv_mlp_apply     optimiser update from dcv_mlp_grads().
 */
int dcv_mlp_forward(dcv_mlp* m, const float* Xn_d, int64_t ld, const int64_t* idx_d, int64_t row0,
                    int32_t batch, int32_t train, void* stream);
double* dcv_mlp_stats(dcv_mlp* m);
int32_t dcv_mlp_stats_len(const dcv_mlp* m);
int dcv_mlp_backward(dcv_mlp* m, const float* Xn_d, int64_t ld, const int64_t* idx_d, int64_t row0,
                     int32_t batch, int64_t global_batch, int32_t train, void* stream);
int dcv_mlp_apply(dcv_mlp* m, void* stream);
/* Data-parallel overlap hook.  With a callback set, dcv_mlp_backward(train = 1) reduces the gradients of layers
 * 1 .. n_layers-1 into dcv_mlp_grads() BEFORE it enqueues the layer-0 weight gradient (the largest product of the
 * step) and calls fn(user) on the host at that point: the caller starts the all-reduce of that part of the buffer --
 * floats [dcv_mlp_param_offset(m, 1, 0), dcv_mlp_num_params) -- on a side stream ordered after the launch stream, so
 * the exchange runs under the layer-0 product; the layer-0 part [0, dcv_mlp_param_offset(m, 1, 0)) is reduced when
 * the call returns.  fn = NULL restores the single reduction. */
int dcv_mlp_set_upper_grads_callback(dcv_mlp* m, void (*fn)(void* user), void* user);
/* One data-parallel step behind ONE entry point: forward, all-reduce of the batch statistics, backward, all-reduce of
 * the gradient buffer, optimiser update -- the sequence a caller would otherwise drive phase by phase (five calls across
 * the language boundary per step).  The collectives are the caller's: fn(user, buf_d, count, dtype, phase) must make the
 * SUM over all ranks of the `count` elements at buf_d (device memory, dtype DCV_DTYPE_F32 / DCV_DTYPE_F64) visible to work
 * that is enqueued on `stream` after it returns (an RCCL / torch.distributed all-reduce ordered against that stream does).
 * phase says what is being exchanged: DCV_DP_STATS (dcv_mlp_stats), DCV_DP_GRADS (the gradient buffer, or its layer-0
 * part), and -- with overlap != 0 and more than one layer -- DCV_DP_UPPER_START for the gradients of layers 1.., handed
 * over BEFORE the layer-0 weight gradient is enqueued: that exchange may complete asynchronously under it and is
 * awaited by the closing call fn(user, NULL, 0, DCV_DTYPE_F32, DCV_DP_WAIT).  fn returns 0, or nonzero to abort the step
 * (dcv_mlp_dp_step then returns DCV_ECALLBACK, after a DCV_DP_WAIT call that joins an exchange already started with
 * DCV_DP_UPPER_START).  train = 0: evaluation step (statistics exchanged, loss logged).
 * Batch normalisation (dcv_mlp_desc.batchnorm) is REFUSED when global_batch != batch (DCV_EINVAL): it would normalise
 * with each rank's local rows and let the running statistics of the ranks drift apart, so N ranks would no longer equal
 * one process on the union batch.
 * Replaces, on the reference side, lightning's DDP hooks around cv_calculator.py:1515-1524 (the reference itself is
 * single-process). */
#define DCV_DTYPE_F32 0
#define DCV_DTYPE_F64 1
#define DCV_DP_STATS 0
#define DCV_DP_GRADS 1
#define DCV_DP_UPPER_START 2
#define DCV_DP_WAIT 3
typedef int (*dcv_allreduce_fn)(void* user, void* buf_d, int64_t count, int32_t dtype, int32_t phase);
int dcv_mlp_dp_step(dcv_mlp* m, const float* Xn_d, int64_t ld, const int64_t* idx_d, int64_t row0, int32_t batch,
                    int64_t global_batch, int32_t train, int32_t overlap, dcv_allreduce_fn fn, void* user, void* stream);
/* ---- RCCL communicator (one process per GPU; RCCL over xGMI inside a node).  EXPERIMENTAL: executed with one rank only
 * (no multi-GPU node has been available to the builder); the default transport of the Python host stays torch.distributed.
 * The collectives of a frame-sharded fit issued
 * by the library itself, in stream order with its kernels.  dcv_comm_unique_id: rank 0 creates the 128-byte id and the
 * caller's bootstrap hands it to every rank; dcv_comm_create: collective over all ranks (ncclCommInitRank on the current
 * device).  dcv_comm_allreduce: in place, op 0 = SUM, 1 = MIN, 2 = MAX, dtype DCV_DTYPE_*, enqueued on `stream`.
 * dcv_comm_dp_allreduce_fn() is an all-reduce callback for dcv_mlp_dp_step with user = the communicator, after
 * dcv_comm_bind_stream(comm, stream) with the step's launch stream: the whole data-parallel step then runs inside the
 * library (the DCV_DP_UPPER_START exchange on a side stream, joined at DCV_DP_WAIT).  librccl.so is opened at run time.
 * Replaces what a torch.distributed / lightning DDP wrapper would do around cv_calculator.py:1515-1524. */
typedef struct dcv_comm dcv_comm;
int dcv_comm_unique_id(void* id_out_128);
int dcv_comm_create(int32_t world, int32_t rank, const void* id_128, dcv_comm** out);
void dcv_comm_destroy(dcv_comm* c);
int dcv_comm_bind_stream(dcv_comm* c, void* stream);
int dcv_comm_allreduce(dcv_comm* c, void* buf_d, int64_t count, int32_t dtype, int32_t op, void* stream);
dcv_allreduce_fn dcv_comm_dp_allreduce_fn(void);
int32_t dcv_comm_world(const dcv_comm* c);
int32_t dcv_comm_rank(const dcv_comm* c);
/* Rank of this engine in a data-parallel run: mixed into the key of the dropout counters, so that ranks holding the same
 * seed mask their local rows independently (default 0). */
int dcv_mlp_set_rank(dcv_mlp* m, int32_t rank);
/* Running statistics of the batch normalisation behind Linear `layer` (dcv_mlp_desc.batchnorm): set != 0 uploads
 * running_mean / running_var (dims[layer + 1] floats each, host) and *num_batches_tracked, set == 0 downloads them.
 * dcv_mlp_set_params resets them to a fresh BatchNorm1d (mean 0, variance 1, 0 batches). */
int dcv_mlp_bn_state(dcv_mlp* m, int32_t layer, float* running_mean_h, float* running_var_h, int64_t* num_batches_tracked,
                     int32_t set, void* stream);
/* Which code path the last forward / step took: 0 = layer by layer (the MFMA block engine), 1 = the fused small-network
 * autoencoder step (one launch: snet.hip), 2 = the fused small-network Deep-TICA kernels (forward + statistics + loss head in
 * one launch, backward in a second: snet_dt.hip).  The fused forms are taken when every weight fits in one CU's LDS
 * (reference-sized networks, cv_calculator.py:2471-2590); DCV_NO_SNET=1 in the environment forces 0. */
int32_t dcv_mlp_last_path(const dcv_mlp* m);
/* Test hook: the batches in the first (largest) grouped launch of the last dcv_mlp_eval_steps call on the block engine, 0 when
 * that call stepped batch by batch or went through the fused small-network kernels. */
int32_t dcv_mlp_last_eval_group(const dcv_mlp* m);
/* Test hook: the reduction workgroups that rode in the layer-0 weight-gradient launch of the last training backward (one-GPU
 * steps of the block engine with the update fused in: every gradient but layer 0's weights is reduced and updated there),
 * 0 when that backward ended on the single reduction launch.  DCV_NO_REDUCE_RIDE=1 in the environment forces 0. */
int32_t dcv_mlp_last_ride(const dcv_mlp* m);
/* Test hook: the kernel that ran the final gradient reduction of the last training backward: 0 = none yet, 1 = the flat-grid
 * ("quad") reduction, 2 = the 4-wave form (DCV_REDUCE_QUAD=0 in the environment), 3 = the 16-wave form (more than 512 weight
 * partials or 1024 bias partials in some layer). */
int32_t dcv_mlp_last_reduce(const dcv_mlp* m);
/* Test hook: the optimiser's state tensors on the device, dcv_mlp_num_params() floats each in the layout of dcv_mlp_params():
 * which = 0 / 1 the two every optimiser owns (Adam: exp_avg / exp_avg_sq), 2 the auxiliary one (amsgrad maximum, centred
 * RMSprop average) or NULL when the optimiser has none. */
float* dcv_mlp_opt_state(dcv_mlp* m, int32_t which);
/* Test hook: post-activation output of Linear `layer` in the last forward (rows x dims[layer + 1] floats, dense).
 * DCV_ESTATE after a fused small-network forward (dcv_mlp_last_path != 0: the activations never left LDS). */
int dcv_mlp_layer_output(dcv_mlp* m, int32_t layer, int64_t rows, float* out_d, void* stream);
/* Convenience for one GPU: forward + backward(train=1) + apply. */
int dcv_mlp_train_step(dcv_mlp* m, const float* Xn_d, int64_t ld, const int64_t* idx_d, int64_t row0,
                       int32_t batch, void* stream);
/* Convenience for one GPU: forward + backward(train=0). */
int dcv_mlp_eval_step(dcv_mlp* m, const float* Xn_d, int64_t ld, const int64_t* idx_d, int64_t row0,
                      int32_t batch, void* stream);
/* The training part of an epoch (the reference's Lightning training loop over the DictLoader, cv_calculator.py:1456-1553 via
 * trainer.fit) with a constant learning rate: `nsteps` training steps, step j on idx_d[j * batch, (j + 1) * batch) -- or the
 * rows row0 + [j * batch, (j + 1) * batch) when idx_d is null -- identical in launches, parameters and loss records to
 * nsteps calls of dcv_mlp_train_step; the caller's per-call cost is paid once. */
int dcv_mlp_train_steps(dcv_mlp* m, const float* Xn_d, int64_t ld, const int64_t* idx_d, int64_t row0,
                        int32_t batch, int32_t nsteps, void* stream);
/* A validation pass (the reference's Lightning validation loop over the DictLoader, cv_calculator.py:1456-1553 via
 * trainer.fit): `nbatches` evaluation steps of `batch` samples each, batch j = idx_d[j * batch, (j + 1) * batch) -- or the
 * rows row0 + [j * batch, (j + 1) * batch) when idx_d is null -- appending the nbatches loss records dcv_mlp_eval_step
 * would append, in batch order, bit for bit.  Networks small enough for the fused kernels (dcv_mlp_last_path 1 / 2) are
 * evaluated many batches per launch.  So is a Deep-TICA network on the block engine (dcv_mlp_last_path 0) without dropout or
 * batch normalisation and with at most 4 outputs: groups of batches, one launch per layer and one for the statistics and loss
 * heads, each batch computed as the single step computes it, in a workspace the engine allocates on the first such pass
 * (at most 256 MB; if that fails the pass steps).  DCV_EVAL_GROUP=0 in the environment (read once) turns the block
 * engine's groups off.  Everything else steps batch by batch.  A ragged last batch is a separate dcv_mlp_eval_step.
 * dcv_mlp_stats() is unspecified afterwards. */
int dcv_mlp_eval_steps(dcv_mlp* m, const float* Xn_d, int64_t ld, const int64_t* idx_d, int64_t row0,
                       int32_t batch, int32_t nbatches, void* stream);

/* Test hook: keep / (1 - p) multipliers (0 or 1 / (1 - p)) that the dropout behind Linear `layer` applies to
 * rows [0, rows) of the batch matrix in training step number `step` (0-based count of training forwards since
 * creation / dcv_mlp_set_params); out_d is rows x dims[layer + 1] floats.  Lets the parity tests hand the oracle
 * the very masks the engine used.  dcv_mlp_dropout_step returns the number of training forwards so far. */
int dcv_mlp_dropout_mask(dcv_mlp* m, int32_t layer, int64_t step, int64_t rows, float* out_d, void* stream);
int64_t dcv_mlp_dropout_step(const dcv_mlp* m);

/* Metrics log: one record of dcv_mlp_log_width() float64 per backward call since the last
 * reset, kept on the device (no host sync inside an epoch).  Record layout:
 *   [loss | batch | Deep-TICA: C0 (d*d) | Ctau symmetrised (d*d) | mean f_t (d)].
 * The host derives eigenvalues / TICA buffers from C0 and Ctau with the reference's own
 * cholesky + eigh recipe -- a d x d solve per record. */
int32_t dcv_mlp_log_width(const dcv_mlp* m);
int dcv_mlp_reset_log(dcv_mlp* m, int32_t capacity, void* stream);
int dcv_mlp_read_log(dcv_mlp* m, double* out_h, int32_t max_records, int32_t* n_records, void* stream);

/* Per-kernel timing for the roofline report: while enabled, HIP events are recorded on the
 * launch stream around the three products of each Linear layer (class = 3*layer + {0 forward,
 * 1 wgrad, 2 dgrad}; level 1 = first layer only, 2 = every layer) for up to max_steps training
 * steps.  dcv_mlp_profile_end synchronises, stops profiling and returns the summed
 * milliseconds and launch counts per class (3*n_layers entries each). */
int dcv_mlp_profile_begin(dcv_mlp* m, int32_t max_steps, int32_t level);
int dcv_mlp_profile_end(dcv_mlp* m, double* ms_h, int32_t* counts_h);
/* Between begin and end: steps issued while paused carry no events (and may go out as graphs), so a timed region can
 * be sampled, e.g. every fourth step.  `paused`: bit 0 = no class is sampled; bits 1 / 2 / 3 = the forward / weight-gradient /
 * input-gradient launches are not sampled (a profiled launch costs the step ~7 us of command-processor work: a caller can
 * stamp the forward product on one step and the weight gradient on another).  Every class counts its own samples (up to
 * max_steps each); dcv_mlp_profile_end reports sums and counts per class. */
int dcv_mlp_profile_pause(dcv_mlp* m, int32_t paused);

/* With DCV_GRAPH=1 in the environment and a non-null stream, dcv_mlp_train_step / forward / backward(train) /
 * eval_step capture their launch sequence into a hipGraph, update the slot's instantiated graph in place (same
 * topology, new arguments) and launch it once.  Off by default: measured, it does not shorten the step on this
 * platform.  Returns how many calls went out as a graph launch. */
int64_t dcv_mlp_graph_launches(const dcv_mlp* m);
int dcv_mlp_set_graph(dcv_mlp* m, int32_t enable);   /* per-engine switch (default: DCV_GRAPH=1 in the environment) */

/* Whole-matrix inference (project / normalize_cv): y = layers[0..latent_layer)(xn) (VAE: the first d = mean columns);
 * Deep-TICA additionally y = (y - tmean) @ tevecs (both d floats / d*d row-major, device,
 * may be NULL); then out = (y - pmean)/prange when given.  minmax_d as in
 * dcv_project_linear.  out_d (n x d) may be NULL. */
int dcv_mlp_infer(dcv_mlp* m, const float* Xn_d, int64_t n, int64_t ld,
                  const float* tmean_d, const float* tevecs_d, const float* pmean_d,
                  const float* prange_d, float* out_d, float* minmax_d, void* stream);

/* Input-gradient pass of the neural sensitivity analysis.  Replaces
 * mlcolvar.explain.sensitivity_analysis(metric="mean_abs_val") as called by
 * NonLinear.sensitivity_analysis, cv_calculator.py:1893-1921: for the n rows given (n <= the
 * engine's row capacity; chunk larger matrices and add the results)
 *   sens[i] = sum_r | d(sum_j cv_j)/d xn[r][i] | * scale[i]          (float64, F values, overwritten)
 * gout_d (dims[latent_layer] floats; VAE: 2d, the log-variance half zero) is the constant gradient of sum_j cv_j with respect to the output of
 * the network layers (the TICA projection and the post-normalisation behind them are affine);
 * scale_d (F floats) is the per-feature factor (dataset std / norm_in range). */
size_t dcv_mlp_input_sensitivity_workspace(const dcv_mlp* m, int64_t n);
int dcv_mlp_input_sensitivity(dcv_mlp* m, const float* Xn_d, int64_t n, int64_t ld, const float* gout_d,
                              const float* scale_d, double* sens_d, void* ws_d, size_t ws_bytes, void* stream);

/* ---------------------------------------------------------------- k-means (a17-a19)
 * Replaces the Lloyd iterations of sklearn.cluster.KMeans as driven by
 * statistics.kmeans_clustering, statistics.py:159-197 (algorithm: SURVEY.md Appendix A.8).
 * One E+M accumulation pass over P (n x d float64, d <= 16, k <= 64); x_i = P_i - offset
 * when offset_d is given (KMeans.fit centres the data by its mean; centres are then
 * expressed in that frame):
 *   label_i = argmin_j (|c_j|^2 - 2 x_i.c_j)   (first minimum wins),
 *   acc_d   = [sums (k*d) | counts (k) | inertia vs `centers` (1) | labels changed (1)] float64,
 * all of which combine over shards by addition.  labels_d (int32) is read (previous labels,
 * for the `changed` count) and overwritten.  HBM-bound: 8*d + 8 bytes per point. */
size_t dcv_kmeans_workspace(int64_t n, int32_t d, int32_t k);
int dcv_kmeans_step(const double* P_d, int64_t n, int32_t d, const double* offset_d /* d or NULL */,
                    const double* centers_d, int32_t k, int32_t* labels_d, double* acc_d, double* mindist_d /* n or NULL */,
                    void* ws_d, size_t ws_bytes, void* stream);

/* k-means++ seeding passes.  Replace the distance / potential arithmetic of sklearn.cluster._kmeans._kmeans_plusplus as
 * reached from statistics.kmeans_clustering, statistics.py:189 (init='k-means++'); the
 * random draws and the sequential float64 cumsum + searchsorted that turn them into candidate rows stay with the caller.
 * Points P (n x d float64, d <= 8), x_i = P_i - offset; dist(x, c) = max(-2 x.c + |c|^2 + |x|^2, 0).
 *   dcv_kmeanspp_update      closest_i = first ? dist(x_i, centre) : min(closest_i, dist(x_i, centre));
 *                            pot_d[0] = sum_i closest_i (adds over shards);
 *   dcv_kmeanspp_potentials  pot_d[t] = sum_i min(closest_i, dist(x_i, cand_t)) for `trials` <= 8 candidate centres
 *                            (trials x d, already in the offset frame). */
size_t dcv_kmeanspp_workspace(int64_t n, int32_t trials);
int dcv_kmeanspp_potentials(const double* P_d, int64_t n, int32_t d, const double* offset_d, const double* cand_d, int32_t trials,
                            const double* closest_d, double* pot_d, void* ws_d, size_t ws_bytes, void* stream);
int dcv_kmeanspp_update(const double* P_d, int64_t n, int32_t d, const double* offset_d, const double* centre_d, int32_t first,
                        double* closest_d, double* pot_d, void* ws_d, size_t ws_bytes, void* stream);

/* ---------------------------------------------------------------- k-selection scores
 * Replace sklearn.metrics calinski_harabasz_score / davies_bouldin_score / silhouette_score as called
 * by statistics.optimize_clustering, statistics.py:73-75, on points P (n x d float64, d <= 16) and
 * int32 labels in [0, k), k <= 64 (other labels are ignored).
 * dcv_label_stats: acc_d = [sums k*d | counts k | sum ||x - c_label||^2 k | sum ||x - c_label|| k]
 * (float64; the last two groups about centers_d (k x d) when given, zero otherwise) -- two calls give
 * the label means and then the dispersions both scores are built from; every group combines over
 * shards by addition.
 * dcv_cluster_dist_sums: S[i][c] = sum over the points j of cluster c of ||Q_i - P_j|| for nq query
 * points against the points sorted by cluster (cluster c = rows [start[c], start[c+1]) of Psorted_d;
 * start_d holds k + 1 int64).  The exact all-pairs silhouette: O(nq * n * d) float64.
 * dcv_silhouette_sum: sum_d[0] = sum of the silhouette sample values of the nq queries (labels
 * qlabels_d), sklearn's definition incl. 0 for singleton clusters; a query with a label outside [0, k)
 * (noise) adds nothing, and start_d describes clusters 0 .. k-1 only (noise rows sorted first: start[0] =
 * their number): divide by the number of queries with a label in [0, k) for the score. */
size_t dcv_label_stats_workspace(int64_t n, int32_t d, int32_t k);
int dcv_label_stats(const double* P_d, int64_t n, int32_t d, const int32_t* labels_d, const double* centers_d /* k*d or NULL */,
                    int32_t k, double* acc_d, void* ws_d, size_t ws_bytes, void* stream);
int dcv_cluster_dist_sums(const double* Q_d, int64_t nq, const double* Psorted_d, const int64_t* start_d, int32_t k, int32_t d,
                          double* S_d /* nq x k */, void* stream);
size_t dcv_silhouette_sum_workspace(int64_t nq);
int dcv_silhouette_sum(const double* S_d, int64_t nq, int32_t k, const int32_t* qlabels_d, const int64_t* start_d,
                       double* sum_d, void* ws_d, size_t ws_bytes, void* stream);

/* Free-energy surface of the projected trajectory (second half).  The reference plots
 * mlcolvar.utils.fes.compute_fes(data, backend="KDEpy", num_samples=num_bins, bandwidth, blocks, bounds) (figures.py:95-98):
 * KDEpy's FFTKDE = linear binning of the points onto the num_bins^d grid, convolution of the grid with the kernel,
 * FES = -kB T log(density + eps).  The streaming stage is the binning: each of the n points (row-major float64, row
 * stride ldp, the d <= 2 columns cols_h) spreads unit weight over the 2^d grid nodes around it.  grid_d receives the
 * bins^d node weights (sum = points inside the bounds; d = 2: grid[i][j], i along the first column); outside_h the
 * number of points outside [lo, hi] (ignored; lo and hi themselves are inside, a non-finite coordinate is outside).  Deterministic (64-bit fixed-point accumulation).  The d-dimensional
 * convolution on the small grid and the logarithm stay with the caller (statistics.compute_fes). */
size_t dcv_linear_binning_workspace(int32_t d, int32_t bins);
int dcv_linear_binning(const double* P_d, int64_t n, int64_t ldp, int32_t d, const int32_t* cols_h, const double* lo_h,
                       const double* hi_h, int32_t bins, double* grid_d, int64_t* outside_h, void* ws_d, size_t ws_bytes, void* stream);

/* Replaces statistics.find_centroids, statistics.py:370-377: for each of the k centroids the
 * index of the nearest of ALL n points under np.linalg.norm (ties -> lowest index).
 * best_d receives k pairs [distance (float64) | row (float64-encoded int64 is avoided:
 * rows_d int64, dist_d float64)] that combine over shards by lexicographic min. */
size_t dcv_nearest_rows_workspace(int64_t n, int32_t d, int32_t k);
int dcv_nearest_rows(const double* P_d, int64_t n, int32_t d, const double* centers_d, int32_t k,
                     int64_t row_offset, double* dist_d, int64_t* rows_d,
                     void* ws_d, size_t ws_bytes, void* stream);

/* Replaces TrajClusterWorkflow.assign_closest_cluster, traj_cluster_workflow.py:207-238:
 * nn_d[i] = index of the training point nearest to supplementary point i (squared
 * Euclidean distance, ties -> lowest index). */
int dcv_nearest_point(const double* train_d, int64_t n_train, const double* sup_d, int64_t n_sup,
                      int32_t d, int64_t* nn_d, void* stream);

/* ---------------------------------------------------------------- hierarchical clustering
 * Replaces sklearn.cluster.AgglomerativeClustering(linkage = complete | average | ward) as called by
 * statistics.cluster_data, statistics.py:146-150, i.e. scipy.cluster.hierarchy.linkage(P, method, "euclidean"):
 * the nearest-neighbour chain over the full float64 distance matrix, with scipy's arithmetic (no fused
 * multiply-adds, correctly rounded sqrt and division), scan order and tie rules, so that Z_h -- (n - 1) x 4
 * float64 in scipy's layout: the two merged ids (smaller first, the i-th merge is node n + i), the height, the
 * size; sorted by height with a stable sort -- EQUALS scipy's.  P (n x d float64 on the device, n >= 2,
 * 1 <= d <= 16) must be finite.  method: 0 complete, 1 average, 2 ward.  searches_h (may be NULL) receives the
 * number of row searches the chain ran (at most 3 (n - 1)).  The workspace holds the SQUARE matrix, rows padded
 * to 16 doubles: 8 n (n + 15) bytes and a little state.  The call synchronises the stream (it reads the merge
 * counter between blocks of steps and the merges at the end).  DCV_EINVAL: bad arguments -- before anything is
 * launched -- or a chain that did not finish (non-finite input); DCV_ENOMEM: workspace too small, nothing
 * launched.  Latency-bound: about 2.8 n chain steps, one launch each (the row update of the previous merge
 * and the search of one row), 6 - 8 us per step. */
size_t dcv_linkage_workspace(int64_t n, int32_t d);
/* the first stage alone (the distance matrix, written into the workspace): what a benchmark times apart */
int dcv_linkage_pdist(const double* P_d, int64_t n, int32_t d, void* ws_d, size_t ws_bytes, void* stream);
int dcv_linkage(const double* P_d, int64_t n, int32_t d, int32_t method, double* Z_h, int64_t* searches_h,
                void* ws_d, size_t ws_bytes, void* stream);

/* ---------------------------------------------------------------- HDBSCAN
 * Replaces the two stages of sklearn.cluster.HDBSCAN (Euclidean, alpha = 1, the kd_tree branch _hdbscan_prims) that
 * touch the points, as statistics.hdbscan_clustering calls them; the condensation of the tree is host work.
 * P is n x d float64 row-major on the device, 2 <= n < 2^31, 1 <= d <= 16, finite.  All distances are
 * sqrt(sum_c (x_c - y_c)^2) with the squares added in coordinate order, no fused multiply-adds and a correctly
 * rounded sqrt, so that both results EQUAL scikit-learn's bit for bit.
 *
 * dcv_core_distances: core_d[i] = the k-th smallest distance from point i to all n points, itself included
 * (NearestNeighbors(n_neighbors = k).kneighbors(P)[0][:, -1]); k = min_samples, 1 <= k <= min(n, 64); k = 1 gives 0.
 * A larger k is DCV_EINVAL before anything is launched.  The workspace is 256 bytes (a status word).
 *
 * dcv_mr_mst: Prim's algorithm from node 0 over mrd(i, j) = max(core[i], core[j], dist(i, j)) with the update and
 * tie rules of sklearn's mst_from_data_matrix (a strictly smaller value replaces a point's running minimum; the
 * new node is the lowest index among the minimal candidates).  src_h / dst_h (int64) and w_h (float64) are HOST
 * arrays of n - 1 entries and receive the edges in Prim order.  One launch per step, n - 1 steps, enqueued in
 * blocks.  The workspace is O(n): 32 n bytes (running minimum, source, in-tree flag, the edges) and about 8 KB of
 * state -- no n x n matrix.
 *
 * Both calls synchronise the stream.  DCV_EINVAL: bad arguments -- before anything is launched -- or points
 * that left a query without k finite distances / a step without a candidate (non-finite input); DCV_ENOMEM:
 * workspace too small, nothing launched.  The *_workspace functions return 0 for arguments out of range. */
size_t dcv_core_distances_workspace(int64_t n, int32_t d, int32_t k);
int dcv_core_distances(const double* P_d, int64_t n, int32_t d, int32_t k, double* core_d, void* ws_d,
                       size_t ws_bytes, void* stream);
size_t dcv_mr_mst_workspace(int64_t n, int32_t d);
int dcv_mr_mst(const double* P_d, int64_t n, int32_t d, const double* core_d, int64_t* src_h, int64_t* dst_h,
               double* w_h, void* ws_d, size_t ws_bytes, void* stream);

/* ---------------------------------------------------------------- building block
 * C[M,N] = op(A).op(B) on the FP32 MFMA engine that the covariance and MLP kernels are built
 * from (v_mfma_f32_32x32x2_f32, exact f32 products, f32 accumulation).  mode 0 (NT):
 * A[M,K] . B[N,K]^T; 1 (NN): A[M,K] . B[K,N]; 2 (TN): A[K,M]^T . B[K,N].  Exposed so that the
 * parity tests can exercise every operand form / tile shape / ragged edge directly. */
int dcv_gemm_f32(int32_t mode, const float* A_d, int64_t lda, const float* B_d, int64_t ldb, float* C_d,
                 int64_t ldc, int64_t M, int64_t N, int64_t K, void* stream);
/* Split-K form of mode 2 as the weight-gradient / covariance paths use it: the K rows are cut into chunks of
 * k_chunk rows, chunk z writes its partial product to slab_d[z] (M x N floats each).  slab_cap is the number of
 * slabs the buffer holds; a launch that needs more returns DCV_ENOMEM without touching memory. */
int dcv_gemm_tn_split(const float* A_d, int64_t lda, const float* B_d, int64_t ldb, float* slab_d, int64_t slab_cap,
                      int64_t M, int64_t N, int64_t K, int64_t k_chunk, void* stream);
/* Test hook: the plans of the block-engine products launched since the last reset, in launch order (a host-side log of fixed
 * capacity, 256 entries; later ones are dropped).  An entry is 9 int32: launch form (0 single product, 1 grouped NT products,
 * 2 weight gradient + input gradient in one launch -- two entries, 3 layer-0 weight gradient + reduction), mode (0 NT, 1 NN,
 * 2 TN), tile rows, tile columns, split (BF16 x 6) flavour, 16-byte loaders, gather-capable kernel form, split-K slabs,
 * chunks of a contraction-split tail tile (0 = whole).  read copies at most cap entries and returns the number recorded.
 * A replayed graph launches without the host wrappers and records nothing. */
void dcv_debug_gemm_log_reset(void);
int32_t dcv_debug_gemm_log_read(int32_t* out, int32_t cap);

#ifdef __cplusplus
}
#endif
#endif /* DCV_H */
