/*
 * lars_hip.h -- C ABI of liblars_hip.so: the MI355X (gfx950) implementation of
 * the per-pixel multispectral index path of lars-uav/lars-image-processing.
 *
 * The reference has no FFI; its boundary for this path is three Python call
 * signatures (file:line in the upstream repository):
 *
 *   fix_white_balance(img_array)              process-images.py:424-447
 *                                             backend-process.py:17-26, process-rgn.py:4-49
 *   calculate_index(img_array, index_type)    process-images.py:449-490
 *   calculate_index(red, green, nir, type)    backend-process.py:28-38
 *   calculate_ndvi(image_path, ...)           process-ndvi.py:5-48   (float64 flavour)
 *   analyze_index(index_array, index_type)    process-images.py:492-513 (+ :651-658, :830-832)
 *   analyze_ndvi_statistics(ndvi_array)       process-ndvi.py:50-73
 *   plt.hist(bins=50, range=(-1,1))           process-ndvi.py:97
 *   imshow(cmap, vmin=-1, vmax=1)             process-images.py:695, backend-process.py:43
 *
 * Each entry point below names the interface it replaces.  A maintainer binds
 * them with ctypes (the shipped binding is
 * lars_image_processing_amd/_ffi.py).
 *
 * Conventions
 *   - plain pointers and sizes only; no C++/torch types.
 *   - every function returns LARS_OK (0) or a negative lars_status; the text of
 *     the last failure on the calling thread is lars_last_error().
 *   - "host entry points" (lars_h_*) take HOST pointers, stage through the
 *     library's device workspace and return when the result is in the caller's
 *     buffer.  They are re-entrant: each calling thread owns a stream and a
 *     workspace.
 *   - "device entry points" (lars_d_*) take DEVICE pointers (lars_malloc) and
 *     enqueue on `stream` (NULL = the calling thread's library stream) without
 *     synchronising; this is what the batched tile path and bench.py use.
 *   - there is no CPU fallback anywhere: without a gfx950 device every compute
 *     entry point fails with LARS_ERR_NO_DEVICE.
 */
#ifndef LARS_HIP_H
#define LARS_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define LARS_ABI_VERSION 1
#define LARS_HIST_BINS 50          /* process-ndvi.py:97 */

typedef enum lars_status {
    LARS_OK = 0,
    LARS_ERR_INVALID = -1,         /* bad argument (shape, dtype, NULL, mask) */
    LARS_ERR_NO_DEVICE = -2,       /* no usable gfx950 GPU / HIP runtime failure at init */
    LARS_ERR_HIP = -3,             /* a HIP call failed; see lars_last_error() */
    LARS_ERR_OOM = -4,             /* device allocation failed */
    LARS_ERR_RCCL = -5,            /* RCCL missing or a collective failed */
    LARS_ERR_UNSUPPORTED = -6
} lars_status;

/* sample types of interleaved images */
#define LARS_U8  1
#define LARS_U16 2

/* index ids / mask bits (process-images.py:466-482) */
#define LARS_NDVI  0               /* (nir - red)   / (nir + red)   */
#define LARS_GNDVI 1               /* (nir - green) / (nir + green) */
#define LARS_NDWI  2               /* (green - nir) / (green + nir) */
#define LARS_MASK_NDVI  1u
#define LARS_MASK_GNDVI 2u
#define LARS_MASK_NDWI  4u
#define LARS_MASK_ALL   7u

/* flags of lars_fused_args.flags */
#define LARS_F_STATS 1u            /* fill stats[tile][index] (min/max/sum/sumsq/above/count) */
#define LARS_F_HIST  2u            /* also the 50-bin histogram (implies LARS_F_STATS) */
#define LARS_F_SUMSQ 4u            /* also the sum of squares, for a standard deviation (implies LARS_F_HIST) */
#define LARS_F_RAW   8u            /* lars_d_fused only: args->stats are running accumulators that the caller has opened with
                                    * lars_d_stats_begin and closes with lars_d_stats_end -- one pair around the launches of a
                                    * batch that is processed in chunks, instead of one pair of small kernels per launch */

/*
 * Order-independent statistics record of one index over one tile (or, after a
 * merge, over many tiles / ranks).  Everything analyze_index (process-images.py
 * :506-512) and analyze_ndvi_statistics (process-ndvi.py:60-71) report except the
 * median follows from it: mean = sum/count, min, max, coverage = above/count*100,
 * std = sqrt(sumsq/count - mean^2).
 *   sum / sumsq : sums of the float32 index values (fixed point 2^-32 accumulation,
 *                 order independent); sum is exact for uint8 tiles and correctly
 *                 rounded to double.  The fused kernel fills sumsq only with
 *                 LARS_F_SUMSQ (it is 0 otherwise).
 *   above       : samples with x > threshold, compared in the sample's own
 *                 precision (float32 against float32(0.2), process-images.py:511).
 *   hist        : numpy.histogram(x, bins=50, range=(-1, 1)) counts.
 */
typedef struct lars_stats {
    double   sum;
    double   sumsq;
    uint64_t count;
    uint64_t above;
    uint64_t nans;
    double   min;                  /* float32 samples widen exactly */
    double   max;
    double   threshold;
    uint32_t index_id;
    uint32_t reserved;
    uint64_t hist[LARS_HIST_BINS];
} lars_stats;

/* ------------------------------------------------------------------ runtime */
int         lars_abi_version(void);
const char *lars_last_error(void);
int         lars_device_count(int *count);
int         lars_set_device(int ordinal);           /* per calling thread; default 0 */
int         lars_get_device(int *ordinal);
int         lars_device_name(char *buf, size_t buflen);
int         lars_malloc(void **dptr, size_t bytes);
int         lars_free(void *dptr);
int         lars_memset(void *dptr, int value, size_t bytes, void *stream);
int         lars_memcpy_h2d(void *dst_dev, const void *src_host, size_t bytes);
int         lars_memcpy_d2h(void *dst_host, const void *src_dev, size_t bytes);
int         lars_memcpy_d2d(void *dst_dev, const void *src_dev, size_t bytes, void *stream);
int         lars_stream_create(void **stream);
int         lars_stream_destroy(void *stream);
int         lars_synchronize(void *stream);         /* NULL = calling thread's library stream */
int         lars_mem_info(size_t *free_bytes, size_t *total_bytes);   /* hipMemGetInfo of the bound device */
int         lars_shutdown(void);                    /* frees the calling thread's workspace */
/* HIP events on a given stream (bench.py times kernels with these) */
int         lars_event_create(void **event);
int         lars_event_destroy(void *event);
int         lars_event_record(void *event, void *stream);
int         lars_event_elapsed_ms(void *start, void *stop, float *ms);   /* synchronises on stop */
/* work enqueued on `stream` after this call waits for `event` (recorded on any stream of the device): how a caller
 * orders passes it overlaps on two streams (hipStreamWaitEvent) */
int         lars_stream_wait_event(void *stream, void *event);

/* --------------------------------------------------------- device entry points */

/* Per-tile, per-channel sample histograms: the pre-pass np.percentile needs
 * (process-images.py:437).  hist is [ntiles][3][nvalues] uint32, nvalues = 256
 * (LARS_U8) or 65536 (LARS_U16); it is zeroed by the call. */
int lars_d_channel_hist(const void *tiles, int64_t ntiles, int64_t npix, int channels,
                        int dtype, uint32_t *hist, void *stream);

/* Histograms -> percentiles (2, 98) -> white-balance table, all on device.
 * table is [ntiles] x lars_wb_table_bytes(dtype) with table[t][c][v] == fix_white_balance()
 * of sample value v in channel c of tile t (process-images.py:437-441: float64
 * arithmetic, clip, float32 store, truncating uint8 cast).  percentiles is
 * [ntiles][3][2] double (may be NULL).  rgn_variant != 0 selects process-rgn.py
 * :25-33 (extra inner clip; same table for integer input, kept for fidelity). */
int lars_d_wb_table(const uint32_t *hist, int64_t ntiles, int64_t npix, int dtype,
                    uint8_t *table, double *percentiles, int rgn_variant, void *stream);

/* Bytes of one tile's white-balance table: 768 for LARS_U8 ([3][256] uint8); for LARS_U16 a blob of
 * 196608 + 4096 bytes: the [3][65536] uint8 table, then its threshold form (uint32 T[3][260],
 * T[c][k] = smallest sample value with table >= k) and double {p2, 255/(p98-p2)}[3] used by the
 * fast uint16 kernel.  wb_table arguments are [ntiles] of these. */
size_t lars_wb_table_bytes(int dtype);

/* The whole white-balance pre-pass of a batch in one call (histogram pass(es) + tables), both
 * sample types.  For LARS_U16 the percentiles come from two radix levels (high-byte histograms,
 * then low-byte histograms of the bins that hold the order statistics) instead of a 65536-bin
 * histogram per channel -- usually in ONE full pass: a subsample predicts a window of values around
 * each percentile, the pass counts the samples below each window and those inside it value by value,
 * and only tiles with an order statistic outside its window take the two radix passes.  Scratch comes
 * from the calling thread's library workspace. */
int lars_d_wb_prepare(const void *tiles, int64_t ntiles, int64_t npix, int channels, int dtype,
                      uint8_t *table, double *percentiles, int rgn_variant, void *stream);
/* Laboratory / test helper: how the last lars_d_wb_prepare on the calling thread used value windows, once its stream has
 * finished.  flags[ntiles] = 1 where a rank lay outside its window (or a mark had none) and the tile took the two radix
 * passes, else 0; windows[ntiles][3][4] = per channel the first value of the 2 % and of the 98 % mark's window and their
 * widths (lo[0], lo[1], wd[0], wd[1]; a width of 0: no window).  LARS_ERR_INVALID unless that call took the value-window
 * route over exactly ntiles tiles (LARS_U16, 3 channels, 4-byte aligned tiles of about 258 k pixels or more, u16_hist_impl
 * other than 1) and no other call on this thread has used the library's scratch since. */
int lars_u16_window_report(int64_t ntiles, uint32_t *flags, uint32_t *windows);

typedef struct lars_fused_args {
    const void    *tiles;          /* [ntiles][h*w][channels] interleaved R,G,NIR(,...) */
    int64_t        ntiles;
    int64_t        npix;           /* h*w */
    int32_t        channels;       /* >= 3 */
    int32_t        dtype;          /* LARS_U8 | LARS_U16 */
    const uint8_t *wb_table;       /* [ntiles] x lars_wb_table_bytes(dtype), or NULL: indices of the raw samples */
    uint32_t       index_mask;     /* LARS_MASK_* */
    uint32_t       flags;          /* LARS_F_* */
    float         *out_index[3];   /* [ntiles][npix] float32 per index, or NULL */
    uint8_t       *out_wb;         /* [ntiles][npix][channels] uint8 (channels >= 3 zero), or NULL */
    uint8_t       *out_rgba[3];    /* [ntiles][npix][4] colormapped index, or NULL */
    const uint8_t *cmap_lut[3];    /* [256][4] RGBA8 table per index (needed where out_rgba set) */
    lars_stats    *stats;          /* [ntiles][3] (entries of unrequested indices untouched), or NULL */
    void          *stream;
} lars_fused_args;

/* The hot path: one pass over interleaved tiles doing band de-interleave,
 * white-balance table lookup, NDVI/GNDVI/NDWI (process-images.py:456-490, IEEE
 * float32), optional float32 / uint8 / RGBA8 outputs and per-tile statistics. */
int lars_d_fused(const lars_fused_args *args);
/* Open / close the statistics records [ntiles][3] of the indices in index_mask for launches with LARS_F_RAW (begin: the
 * accumulators of lars_d_fused's own prologue; end: sums, count, minimum and maximum in their final form). */
int lars_d_stats_begin(lars_stats *stats, int64_t ntiles, uint32_t index_mask, void *stream);
int lars_d_stats_end(lars_stats *stats, int64_t ntiles, uint32_t index_mask, int64_t npix, void *stream);

/* White-balance tables of a batch of LARS_U8 tiles from a SAMPLE of every tile (csrc/wb_predict.hip), proven exact while the
 * planes are written.  lars_d_wb_predict stands where lars_d_channel_hist + lars_d_wb_table stood: per tile it counts a
 * fraction of the tile (whole 4 KiB segments at hashed positions), takes per channel and mark the value whose bin holds the
 * mark in the sample's CDF, and calls the mark confident when both edges of that bin lie k standard errors away from it (the
 * error measured between 16 interleaved groups of segments).  A tile whose six marks are confident gets percentiles and table
 * from the predicted values and is PREDICTED; every other tile takes the exact pass in the same call.  *predicted = 1 when the
 * predictor ran at all (3-channel 4-byte aligned tiles of at least wb_predict_min_pixels pixels, knob wb_predict not 0), else
 * the call was the exact pre-pass.  The hist rows of predicted tiles are zero until something counts them.
 *   lars_d_fused_verified   lars_d_fused over tiles [tile_start, tile_start + args->ntiles) of that batch (args->wb_table,
 *                           args->stats and the outputs start at tile_start as ever; v names the batch's arrays).  Where a
 *                           verifying kernel exists (uint8 RGNir fast path, white balance, at most basic statistics) the launch
 *                           counts, per channel and over all pixels, the samples below and up to each predicted value; a tile
 *                           whose counts do not prove all six percentiles is repaired right behind it on the same stream: exact
 *                           histogram pass, tables, its statistics records opened again, the launch repeated for it -- plain
 *                           kernels whose blocks return early, each evaluating the counts itself.  Elsewhere the predicted tiles
 *                           of the range take the exact pass first.  Either way everything the call leaves is exact.
 *   lars_d_wb_settle        the exact pass for every tile still predicted: what any other reader of the tables calls first.
 *   lars_wb_predict_report  (tiles the last lars_d_wb_predict called confident, tiles among them a verified launch has
 *                           repaired since), after the stream has finished.
 * scratch: lars_wb_predict_scratch_bytes(ntiles) bytes of device memory owned by the caller, the same for all four calls. */
typedef struct lars_wb_verify {
    void     *scratch;
    int64_t   batch_tiles;         /* tiles of the batch the scratch, hist and percentiles belong to */
    int64_t   tile_start;          /* the launch's first tile inside the batch */
    uint32_t *hist;                /* [batch_tiles][3][256] */
    double   *percentiles;         /* [batch_tiles][3][2] */
    int32_t   rgn_variant;         /* flavour of the tables (lars_d_wb_table) */
} lars_wb_verify;
size_t lars_wb_predict_scratch_bytes(int64_t ntiles);
int lars_d_wb_predict(const void *tiles, int64_t ntiles, int64_t npix, int channels, int dtype, uint32_t *hist, uint8_t *table,
                      double *percentiles, int rgn_variant, void *scratch, int *predicted, void *stream);
int lars_d_fused_verified(const lars_fused_args *args, const lars_wb_verify *v);
int lars_d_wb_settle(const void *tiles, int64_t ntiles, int64_t npix, uint32_t *hist, uint8_t *table, double *percentiles,
                     int rgn_variant, void *scratch, void *stream);
int lars_wb_predict_report(const void *scratch, int64_t ntiles, int64_t *confident, int64_t *missed);

/* float32 band planes -> index, backend-process.py:28-38 (literal formula with
 * the float32 epsilon add and the clip; any float input). */
int lars_d_index_planes_f32(const float *red, const float *green, const float *nir,
                            int64_t n, int index_id, float *out, void *stream);

/* interleaved image -> float64 NDVI, process-ndvi.py:18-31 */
int lars_d_ndvi_f64(const void *img, int64_t npix, int channels, int dtype,
                    double *out, void *stream);

/* Statistics of an arbitrary float32 / float64 array (process-images.py:506-512,
 * process-ndvi.py:60-71).  want_hist adds the 50-bin histogram. */
int lars_d_array_stats_f32(const float *x, int64_t n, float threshold, int want_hist,
                           lars_stats *out_dev, void *stream);
int lars_d_array_stats_f64(const double *x, int64_t n, double threshold, int want_hist,
                           lars_stats *out_dev, double *out_sumsqdev_dev, void *stream);

/* np.median by radix select on device: writes the two middle order statistics
 * ((n-1)/2 and n/2) to out_dev[0..1]. scratch must hold lars_select_scratch_bytes(). */
size_t lars_select_scratch_bytes(void);
int lars_d_median_pair_f32(const float *x, int64_t n, float *out_dev, void *scratch, void *stream);
int lars_d_median_pair_f64(const double *x, int64_t n, double *out_dev, void *scratch, void *stream);
/* Batched: `items` arrays of n float32 values, `stride` values apart (the index planes of a batch of
 * tiles); out_dev is [items][2]; scratch must hold items * lars_select_scratch_bytes(). */
int lars_d_median_pair_batch_f32(const float *x, int64_t n, int64_t items, int64_t stride, float *out_dev,
                                 void *scratch, void *stream);

/* One pass of the two-level select over the index values of a batch WITHOUT the planes in memory (exact batch /
 * global medians): the NDVI and GNDVI quotients of every pixel are recomputed from the
 * uint8 tiles.  Position of a value: t = float32 fma(x, 1023.5, 3071.5) in [2048, 4095]; its 23 mantissa bits are
 * 11 bits of bucket and 12 bits of fraction.  first == 1: each value is counted in its bucket, under track 0 (first == 3:
 * the same over a 1/16 subsample of the pixels -- the prediction of the window below).
 * first == 0: per stream s and track k, the values of bucket[2s+k] are counted in slot (fraction >> 2) (1024 slots);
 * when both tracks of BOTH streams share their bucket only track 0 is counted.  A slot holds one distinct value
 * (two different quotients of bytes are >= 1/(510 * 509) apart = 16 units of the fraction).
 * first == 2: ONE pass instead of those two where a predicted window holds the ranks.  Slots sigma(x) = round(x * 524032);
 * (int32) bucket[2s] is the first slot ws of stream s's window of 1920 slots (3.75 buckets); under track 0 of stream s
 * words 0..63 together count the values below the window, words 64..1983 its slots, words 1984..2047 the values above.
 * hist is uint64[2 streams][2 tracks][2048], accumulated with atomics (zero it first).  NDWI = -GNDVI shares
 * GNDVI's order statistics. */
int lars_d_quotient_select_hist(const void *tiles, int64_t ntiles, int64_t npix, int channels, int dtype,
                                const uint8_t *wb_table, uint32_t streams /* bit 0 NDVI, bit 1 GNDVI (and NDWI) */, int first,
                                const uint32_t bucket[4], uint64_t *hist, void *stream);
/* np.median of the NDVI and GNDVI planes of EVERY tile without writing a plane: per-tile histograms, the picks and the
 * value look-up on the device.  Usually ONE full pass: a subsample predicts a window per tile and stream, a window pass
 * (first == 2 above, per tile) counts it, and only tiles whose ranks fall outside take the two classic passes -- to find
 * out which, the call waits for its stream once (one word comes back to the host; lars_set_tuning("selq_window", 0)
 * = always the two passes, no wait).  out_pairs is float[ntiles][2 streams: NDVI, GNDVI][2]: the two middle order
 * statistics (median = their float32 mean; NDWI's median is -GNDVI's).  scratch holds
 * lars_quotient_median_scratch_bytes(ntiles). */
size_t lars_quotient_median_scratch_bytes(int64_t ntiles);
/* The statistics of lars_d_fused (a->stats, LARS_F_HIST honoured; index_mask = one index or all three; no
 * output planes) AND those medians in one call: the statistics kernel also counts the select's first
 * pass, so the tiles are read twice (three times with the white-balance histogram pass).  Streams the mask does not ask for come back
 * as NaN pairs.  With plain LARS_F_STATS the select passes are usually not needed at all: a subsample predicts a window per
 * tile and stream, the statistics kernel counts the values below it and the slots inside it instead of the buckets, and only
 * tiles whose ranks fall outside their window take the two classic passes -- to find out which, this call waits for its
 * stream once (one word comes back to the host). */
int lars_d_stats_medians(const lars_fused_args *a, float *out_pairs, void *scratch);
int lars_d_quotient_median_pairs(const void *tiles, int64_t ntiles, int64_t npix, int channels, int dtype,
                                 const uint8_t *wb_table, uint32_t streams /* bit 0 NDVI, bit 1 GNDVI; others come back NaN */,
                                 float *out_pairs, void *scratch, void *stream);

/* The statistics of lars_d_fused -- and the exact medians of lars_d_stats_medians -- from ONE read of the tiles, with the
 * white balance's own percentile pre-pass inside (csrc/joint.hip): every figure analyze_index reports
 * (process-images.py:506-512: mean, median, min, max, coverage), the 50-bin histogram (process-ndvi.py:97) and
 * np.percentile(ch, (2, 98)) of fix_white_balance (process-images.py:437) is a function of how often each pair of raw
 * bytes (nir, red) resp. (nir, green) occurs.  A counting kernel builds those 2 x 65536 counts per tile in LDS (no table
 * look-up, no quotient per pixel), a second kernel derives channel histograms -> percentiles -> tables -> records ->
 * medians from them.  The records are bit-identical to lars_d_fused's -- except the optional sum of squares (LARS_F_SUMSQ:
 * count x value^2 per cell here, value^2 per pixel there; they agree to a few units of 2^-32) -- the medians to np.median.
 *   a             uint8 tiles with 3 channels (RGNir; 4-byte aligned) or 4 (RGBA, alpha ignored; 16-byte aligned), npix < 2^32
 *                 (the per-cell counts are uint32); index_mask any non-empty subset; LARS_F_HIST / LARS_F_SUMSQ honoured; no
 *                 output planes; a->stats [ntiles][3] receives final records (unrequested indices untouched);
 *                 a->wb_table, if not NULL, is an OUTPUT here: [ntiles][3][256] tables of the channels the mask needs
 *                 (NIR and red for NDVI, NIR and green for GNDVI / NDWI)
 *   white_balance 0: indices of the raw samples (calculate_index without fix_white_balance); 1: percentile white balance
 *   percentiles   [ntiles][3][2] double or NULL, hist [ntiles][3][256] or NULL: outputs, same channels as the tables.
 *                 With hist == NULL, white_balance != 0, both value streams in the mask and tiles of >= 2^20 pixels the call may
 *                 count a tile on WINDOWED tables (csrc/joint_win.hip): red and green clamped to a window around their
 *                 percentiles -- fix_white_balance maps everything at or below p2 to 0 and at or above p98 to 255
 *                 (process-images.py:438), so the records, percentiles, tables and medians are the same bits -- which lets both pair
 *                 tables of a tile chunk live in ONE workgroup's LDS: one reader per byte instead of two.  A subsample predicts
 *                 the windows, the exact percentiles check them, a tile whose window missed is counted again on full tables
 *                 (lars_set_tuning("joint_window", 0) = never windowed; 2 = windows that miss on purpose).  Where red and green
 *                 windows with NIR whole do not fit (more than 306 rows) NIR gets a window too -- it is white-balanced through
 *                 its own percentiles like the others -- and rows shrink to its width: three windows of up to about 196 values
 *                 each still share one workgroup.  Channel histograms cannot be had from clamped counts: asking for hist keeps
 *                 the full tables
 *   out_pairs     float[ntiles][2 streams: NDVI, GNDVI][2] or NULL: the two middle order statistics (median = their
 *                 float32 mean; NDWI's is -GNDVI's); a stream the mask does not need comes back as NaN
 *   scratch       scratch_bytes >= lars_joint_scratch_bytes(ntiles, npix, index_mask) bytes of device memory; its first word
 *                 is an error flag the launch leaves at 0 (1 = a workgroup's hand-over list overflowed: cannot happen while a
 *                 workgroup counts at most 2^24 pixels, which the chunking guarantees) */
size_t lars_joint_scratch_bytes(int64_t ntiles, int64_t npix, uint32_t index_mask);
int lars_d_stats_joint(const lars_fused_args *a, int white_balance, int rgn_variant, double *percentiles, uint32_t *hist,
                       float *out_pairs, void *scratch, size_t scratch_bytes);
/* How the last lars_d_stats_joint on `scratch` used windowed tables (csrc/joint_win.hip), once its stream has finished:
 * *windowed = tiles counted by one reader on windowed tables, *recounted = tiles among them whose window missed a percentile's
 * order statistic and which were counted again on full tables.  Both 0 after a call that did not qualify (see above). */
int lars_joint_window_report(const void *scratch, int64_t ntiles, int64_t *windowed, int64_t *recounted);
/* ... and by table form: counts[0] = tiles counted on full tables (two readers), counts[1] = on windowed red and green rows with NIR
 * whole, counts[2] = on three windows (recounted tiles are listed under the form they were first counted on). */
int lars_joint_window_modes(const void *scratch, int64_t ntiles, int64_t counts[3]);

/* classification mask (see lars_h_threshold_mask_f32); x 16-byte, out_mask 4-byte aligned */
int lars_d_threshold_mask_f32(const float *x, int64_t n, float threshold, uint8_t *out_mask, void *stream);

/* float32 index -> RGBA8: LUT[min(int((x + 1f) * 128f), 255)], the per-pixel
 * mapping of imshow(cmap, vmin=-1, vmax=1) (process-images.py:695). */
int lars_d_colormap_f32(const float *x, int64_t n, const uint8_t *lut_rgba, uint8_t *out_rgba,
                        void *stream);
/* ... and only the entry min(int((x + 1f) * 128f), 255) of every sample, one byte each (x 16-byte, out_entry 4-byte aligned). */
int lars_d_colormap_entry_f32(const float *x, int64_t n, uint8_t *out_entry, void *stream);

/* ---- registration and change detection ---- */
/* skimage.color.rgb2gray of a uint8 [npix][3] image (process-images.py:538-546) into the real parts of a
 * complex128 buffer [npix][2] (imaginary parts 0); channels == 1: the sample value itself. */
int lars_d_gray_c128(const uint8_t *img, int64_t npix, int channels, double *out_c128, void *stream);
/* skimage.registration.phase_cross_correlation(fixed, moving) with its defaults (process-images.py:549):
 * FFT cross-power spectrum / max(|.|, 100 eps) -> inverse FFT -> argmax |.| -> signed shift.  Both
 * [h][w] complex128 buffers are overwritten.  shift_dev receives {dy, dx}; scratch holds
 * lars_phase_scratch_bytes().  The FFTs run in rocFFT via libhipfft.so, loaded on first use. */
size_t lars_phase_scratch_bytes(void);
int lars_d_phase_correlation(double *fixed_c128, double *moving_c128, int64_t h, int64_t w, int64_t *shift_dev,
                             void *scratch, void *stream);
/* scipy.ndimage.shift(img, (dy, dx, 0), order=1, mode='reflect') for the integer shift in shift_dev
 * (process-images.py:557); out must not alias img. */
int lars_d_shift_reflect_u8(const uint8_t *img, int64_t h, int64_t w, int channels, const int64_t *shift_dev,
                            uint8_t *out, void *stream);
/* diff = late - early (process-images.py:923) */
int lars_d_diff_f32(const float *early, const float *late, int64_t n, float *out_diff, void *stream);
/* RGBA8 of cmap(Normalize(vmin, vmax)(x), bytes=True): the per-pixel mapping of
 * imshow(x, cmap, vmin, vmax) -- e.g. the change map's bwr, -0.5, 0.5 (process-images.py:956). */
int lars_d_colormap_norm_f32(const float *x, int64_t n, float vmin, float vmax, const uint8_t *lut_rgba,
                             uint8_t *out_rgba, void *stream);

/* Synthetic RGNir tiles generated in HBM (bench / tests): counter hash of
 * (seed, tile, word); profile 0 = uniform bytes, 1 = vegetation-like squeeze. */
int lars_d_synth_u8(uint8_t *tiles, int64_t ntiles, int64_t first_tile, int64_t npix, int channels,
                    uint32_t seed, int profile, void *stream);

/* Tuning knobs (per process): "fused_impl" 0 (auto)|1|2, "hist_impl" 1|2, "nt_stores" 0|1, "blocks_per_tile" 0 = automatic
 * (also the chunks per tile of lars_d_stats_joint), "joint_depth" 4|6|8|12 loads in flight per lane of the counting kernel,
 * "joint_window" 1 (windowed pair tables where they fit: lars_d_stats_joint)|0 (never)|2 (windows that miss on purpose: exercises the
 * recount; tiles of any size)|3 (as 1 for tiles of any size)|4 (three windows -- NIR as well -- wherever they fit, before two are tried; tiles
 * of any size)|5 (as 4 with NIR windows that miss on purpose), "joint_win_depth" 4|5|6|12|15 loads in flight per lane of the windowed counting kernel,
 * "u16_hist_impl" 5 (uint16 percentiles usually from ONE full pass: per channel and mark the count of the samples below a window
 * predicted from a subsample and the histogram inside it; a tile whose window missed takes the two radix passes)|1 (always the two
 * radix passes)|3 (windows that miss on purpose: exercises the fall-back),
 * "selq_window" 1 (one-pass medians)|0 (always two select passes)|2 (wrong windows: exercises the fallback), "selq_list_wgs"
 * workgroups per select pass over the tiles a window missed (0 = 2048), "jpeg_subseq_bits" 32 .. 65536: the bits of entropy data one
 * lane of the JPEG decoder takes (lars_d_decode_jpeg_u8; 32 = the longest code plus its extra bits, rounded up).
 * The knob load_policy (0 .. 2) is the cache policy of the kernels' streaming tile loads: 0 = each kernel's measured choice
 * (profiles/load_policy_kernels.txt), 1 = plain loads everywhere, 2 = non-temporal (nt) loads everywhere.
 * The knob wb_predict is how lars_d_wb_predict decides: 1 = tables predicted from a sample and proven while the planes are written,
 * 0 = never (the exact pre-pass), 2 = every prediction one value off (every confident tile misses and is repaired: a test hook),
 * 3 = the confidence gate always passes (test hook); wb_predict_sixteenths 2 .. 4 = sixteenths of a tile it samples,
 * wb_predict_k 1 .. 16 = standard errors a mark must keep from the edges of its bin, wb_predict_min_pixels = smaller tiles always
 * take the exact pass.
 * Results never depend on them.  Read-only:
 * "last_fused_kernel" = the kernel family the last lars_d_fused launched (1 k_fused_u8c3, 2 k_fused_v2, 3 its uint16 form,
 * 4 k_fused_generic: one pixel per lane, 5 k_fused_u8c3 for RGBA uint8 tiles), "jpeg_last_rounds" = the synchronisation rounds
 * that decoded anything in the last lars_h_decode_jpeg_u8 / lars_h_thumbnail_jpeg_u8 of the process (+100 when the serial finish ran). */
int lars_set_tuning(const char *key, int value);
int lars_get_tuning(const char *key, int *value);

/* Build-time switches of the kernel sources this library was compiled with: 0 for the product (what `make` builds and the
 * package loads).  Laboratory builds (csrc/Makefile `lablayout`, `EXTRA=-D...`) report what they changed: the plane-layout knob
 * (one more kernel argument: other register counts), IEEE division instead of rcp + fma (same results, slower), another
 * geometry of the statistics-only kernels.  Needs no device. */
#define LARS_BUILD_LAB_LAYOUT 1u
#define LARS_BUILD_IEEE_DIV 2u
#define LARS_BUILD_COUNT_MODE 4u        /* retired and never set (vector coverage counters; the switch left the sources): do not reuse 4u */
#define LARS_BUILD_STATS_GEOMETRY 8u
unsigned int lars_build_flags(void);

/* Device self-check: number of (num, den) pairs, 1 <= den <= max_den, |num| <= den,
 * for which the kernels' rcp+fma quotient differs from IEEE float32 division
 * (must be 0; tests run it for the uint8 and the uint16 operand ranges). */
int lars_d_quot_selfcheck(uint32_t max_den, uint64_t *mismatches, uint32_t first_bad[2]);

/* Fold n records (same index) into one: sums add, min/max fold, histograms add. */
int lars_stats_merge(const lars_stats *records, int64_t n, lars_stats *out);
/* The same fold on the device, per index over the tiles of a batch: tile_records [ntiles][3] (final form) -> out[3]
 * (entries of indices outside index_mask untouched), bit-identical to lars_stats_merge over tile_records[:, k] in tile
 * order.  The three records are what a rank hands to lars_comm_allreduce_stats(..., is_device = 1): nothing but 3 x 472
 * bytes leaves the device per step. */
int lars_d_stats_fold(const lars_stats *tile_records, int64_t ntiles, uint32_t index_mask, lars_stats *out, void *stream);

/* ----------------------------------------------------------- host entry points */

/* fix_white_balance(img_array) -- process-images.py:424-447 (variant 0),
 * backend-process.py:17-26 (variant 0), process-rgn.py:25-44 (variant 1).
 * img/out are host [h][w][channels]; out is uint8 with channels >= 3 zeroed. */
int lars_h_fix_white_balance(const void *img, int64_t h, int64_t w, int channels, int dtype,
                             int variant, uint8_t *out, double *percentiles /* [3][2] or NULL */);
/* The same function for any other sample type: process-images.py:431 casts whatever it is given with
 * astype(np.float32) before anything else, so the caller hands over that float32 image.  np.percentile's order
 * statistics come from an exact radix select, numpy's `_lerp` (float32 difference, float64 blend) and the float64
 * stretch / float32 store / truncating cast of :438-441 run on the device. */
int lars_h_fix_white_balance_f32(const float *img, int64_t h, int64_t w, int channels, uint8_t *out,
                                 double *percentiles /* [3][2] or NULL */);

/* calculate_index(img_array, index_type) -- process-images.py:449-490.
 * Several indices in one pass: out[k] is host [h][w] float32 or NULL. */
int lars_h_calculate_index(const void *img, int64_t h, int64_t w, int channels, int dtype,
                           uint32_t index_mask, float *const out[3],
                           lars_stats *stats /* [3] or NULL */, int want_hist);

/* calculate_index(red, green, nir, index_type) -- backend-process.py:28-38 */
int lars_h_calculate_index_planes(const float *red, const float *green, const float *nir,
                                  int64_t n, int index_id, float *out);

/* calculate_ndvi maths -- process-ndvi.py:18-31 (float64 out) */
int lars_h_ndvi_f64(const void *img, int64_t h, int64_t w, int channels, int dtype, double *out);

/* analyze_index / analyze_ndvi_statistics on a host array: stats + the two
 * middle order statistics (median = their mean) + sum of squared deviations
 * from the mean (np.std, float64 flavour). */
int lars_h_analyze_f32(const float *x, int64_t n, float threshold, int want_hist,
                       lars_stats *out, float median_pair[2]);
int lars_h_analyze_f64(const double *x, int64_t n, double threshold, int want_hist,
                       lars_stats *out, double median_pair[2], double *sumsqdev);

/* Whole reference pipeline for one host image in one upload:
 * white balance -> requested indices -> statistics (+ medians) -> optional
 * RGBA8 colormaps.  Any output pointer may be NULL.  out_rgba[k] with cmap_lut[k] == NULL (or cmap_lut == NULL) receives the
 * colormap ENTRY of every pixel instead -- [h][w] uint8, min(int((x + 1f) * 128f), 255): the pixels of a palette image whose
 * palette is the colormap (backend-process.py:40-47, process-images.py:690-695 per pixel) -- one byte per pixel over PCIe. */
int lars_h_process_image(const void *img, int64_t h, int64_t w, int channels, int dtype,
                         int apply_wb, uint32_t index_mask, int want_hist,
                         uint8_t *out_wb, float *const out_index[3],
                         lars_stats *stats /* [3] */, float *medians /* [3][2] */,
                         uint8_t *const out_rgba[3], const uint8_t *const cmap_lut[3]);

int lars_h_colormap_f32(const float *x, int64_t n, const uint8_t *lut_rgba, uint8_t *out_rgba);
/* classification mask: out_mask[i] = index[i] > threshold in float32 (the array np.mean averages for the
 * coverage figures, process-images.py:511 / :657); 1 byte per sample, 0 or 1 */
int lars_h_threshold_mask_f32(const float *x, int64_t n, float threshold, uint8_t *out_mask);

/* preprocess_large_image -- process-images.py:398-422: PIL.Image.resize((new_w, new_h), LANCZOS) of a
 * uint8 image with 1, 3 or 4 (RGBA, premultiplied-alpha path) channels, bit-identical to Pillow's
 * fixed-point resampler.  out is host [new_h][new_w][channels]. */
int lars_h_resize_lanczos_u8(const uint8_t *img, int64_t h, int64_t w, int channels, int64_t new_h, int64_t new_w,
                             uint8_t *out);
/* gallery thumbnail -- process-images.py:186-189: img.thumbnail(size, Image.Resampling.LANCZOS, reducing_gap), bit-identical
 * to Pillow, on the plan lars_image_processing_amd.api.thumbnail_plan computes: img is the decoded (after draft) uint8 image
 * [h][w][channels] (1 L, 3 RGB, 4 RGBA: premultiplied alpha, as Pillow resizes RGBA); Image.reduce((fx, fy)) over
 * reduce_box = {x0, y0, x1, y1} (skipped when fx = fy = 1 and the box is the whole image); then the LANCZOS passes from
 * the float box = {x0, y0, x1, y1} of the reduced image to new_w x new_h, an axis only where it changes, vertical first
 * when vertical_first != 0 (Image.resize's tall-image branch).  out is host [new_h][new_w][channels]. */
int lars_h_thumbnail_u8(const uint8_t *img, int64_t h, int64_t w, int channels, int fx, int fy, const int reduce_box[4],
                        const float box[4], int64_t new_h, int64_t new_w, int vertical_first, uint8_t *out);

/* align_images -- process-images.py:515-565 for two uint8 images of the same shape ([h][w][3] or [h][w]):
 * out_aligned = moving registered onto fixed, shift = {dy, dx} (what phase_cross_correlation returns). */
int lars_h_align_images(const uint8_t *fixed, const uint8_t *moving, int64_t h, int64_t w, int channels,
                        uint8_t *out_aligned, double shift[2]);
/* create_change_detection_visualization's arithmetic -- process-images.py:885-923 and :956 -- in one upload:
 * optional white balance of either image, optional registration of the late image, the index of both,
 * diff = late - early and its colormap.  Any output pointer may be NULL. */
int lars_h_change_detection(const uint8_t *early, const uint8_t *late, int64_t h, int64_t w, int channels,
                            int wb_early, int wb_late, int align, int index_id,
                            float *out_early, float *out_late, float *out_diff,
                            uint8_t *out_rgba_diff, const uint8_t *lut_rgba, float vmin, float vmax,
                            uint8_t *out_aligned_late, double shift[2]);
int lars_h_colormap_norm_f32(const float *x, int64_t n, float vmin, float vmax, const uint8_t *lut_rgba,
                             uint8_t *out_rgba);

/* PNG files of 8-bit pictures, built on the device -- the Image.fromarray(x).save(png) that ends every index picture of the
 * batch driver (backend-process.py:49-73) and of the ZIP export (process-images.py:567-617).  img is uint8 [h][w][channels]:
 * 1 (L, or P when palette_rgba is given: palette_len RGBA entries, written as PLTE + tRNS), 3 (RGB) or 4 (RGBA); 8 bits,
 * no interlace, 1 <= h, w <= 2^24.  The pixels decode exactly to img; the compressed bytes are this library's own (libpng's
 * filter heuristic per row, one literal-only dynamic Huffman block per 32 KiB of filtered data, one IDAT chunk each).  The
 * same input always gives the same bytes.  With the knob deflate_matching at 1 (lars_set_tuning: 0 or 1, default 0) the coder
 * searches every 32 KiB for repeats and writes a block of literals and length / distance pairs where that is shorter than both
 * other forms; where it is not, the 32 KiB are coded as at 0.  Same pixels, same bound, another (never a longer) file.
 * lars_png_bound: the largest file any input of that shape can give (0 for a shape that cannot be encoded); pure host code.
 * lars_png_scratch_bytes: device scratch of lars_d_encode_png_u8.
 * lars_d_encode_png_u8: device img / palette_rgba / out (out_cap >= lars_png_bound) / scratch; enqueues on stream and
 * writes the file's length to the device int64 *out_len_dev.
 * lars_h_encode_png_u8: host img / palette_rgba / out; one upload, then the length, then out_len bytes into out. */
size_t lars_png_bound(int64_t h, int64_t w, int channels);
size_t lars_png_scratch_bytes(int64_t h, int64_t w, int channels);
int lars_d_encode_png_u8(const uint8_t *img, int64_t h, int64_t w, int channels, const uint8_t *palette_rgba, int palette_len,
                         uint8_t *out, size_t out_cap, int64_t *out_len_dev, void *scratch, void *stream);
int lars_h_encode_png_u8(const uint8_t *img, int64_t h, int64_t w, int channels, const uint8_t *palette_rgba, int palette_len,
                         uint8_t *out, size_t out_cap, int64_t *out_len);
/* lars_h_process_image with every requested index picture encoded as a PNG on the device (backend-process.py:49-73 per
 * file): png_mode 1 encodes the RGBA colormap picture of cmap_lut[k], png_mode 2 a palette (P) picture of the colormap
 * entries with cmap_lut[k] as its 256-entry palette.  cmap_lut[k] and out_png[k] (host, png_cap bytes, at least
 * lars_png_bound(h, w, 4) or (h, w, 1)) are needed for every index in index_mask; png_len[k] receives the file's length.
 * The colormap planes never leave the device. */
int lars_h_process_image_png(const void *img, int64_t h, int64_t w, int channels, int dtype,
                             int apply_wb, uint32_t index_mask, int want_hist,
                             uint8_t *out_wb, float *const out_index[3],
                             lars_stats *stats /* [3] */, float *medians /* [3][2] */,
                             const uint8_t *const cmap_lut[3], int png_mode,
                             uint8_t *const out_png[3], size_t png_cap, int64_t png_len[3]);

/* PNG files decoded on the device -- the Image.open(io.BytesIO(img_bytes)) + np.array(img) of load_image_from_db
 * (process-images.py:181-193) and the img.thumbnail((400, 400), LANCZOS) after it (process-images.py:186-189).
 * Covered: bit depth 8, no interlace, colour types 0 (L), 2 (RGB), 3 (P: the palette indices), 4 (LA), 6 (RGBA); the
 * pixels come out as Pillow's np.asarray gives them, uint8 [h][w][channels].  IDAT CRCs and the Adler-32 trailer are always
 * checked (Pillow checks neither) whenever the stream decodes to exactly the image's bytes.  A stream that decodes to more
 * (data past the image, which Pillow ignores) has its extra bytes dropped, not stored -- their length is bounded only by
 * 1032 x the compressed size -- so the Adler-32 over all of them cannot be formed and that trailer is not checked.
 * lars_png_info: pure host code.  Validates the chunk layout of file[0..len) (signature, IHDR first, IDATs consecutive,
 * IEND, every chunk inside the file, the CRC of every chunk but IDAT) and fills info[LARS_PNG_INFO_N] = { width, height,
 * bit depth, colour type, interlace, channels, IDAT payload bytes, IDAT chunks, APNG, supported }; idat_table (may be NULL
 * with idat_cap 0) receives { payload offset, payload length } of the first idat_cap IDAT chunks.
 * lars_png_decode_scratch_bytes: device scratch of lars_d_decode_png_u8 (0 for a shape it cannot decode).
 * lars_d_decode_png_u8: device file / idat_table (info[LARS_PNG_INFO_IDAT_COUNT] pairs, as lars_png_info gave them) / out (h * w * channels bytes)
 * / scratch; enqueues on stream and writes { LARS_PNGD_* status, detail } to the device int32 status_dev[2].
 * lars_h_decode_png_u8: host file in, host pixels out (out_cap >= h * w * channels); one upload, one download.
 * lars_h_thumbnail_png_u8: host file in (modes L, RGB, RGBA), lars_h_thumbnail_u8's plan numbers, host thumbnail out; the
 * decoded pixels never leave the device. */
#define LARS_PNG_INFO_N 10
enum {                           /* positions in lars_png_info's info[] */
    LARS_PNG_INFO_WIDTH = 0,
    LARS_PNG_INFO_HEIGHT = 1,
    LARS_PNG_INFO_BIT_DEPTH = 2,
    LARS_PNG_INFO_COLOR_TYPE = 3,
    LARS_PNG_INFO_INTERLACE = 4,
    LARS_PNG_INFO_CHANNELS = 5,
    LARS_PNG_INFO_IDAT_BYTES = 6,
    LARS_PNG_INFO_IDAT_COUNT = 7,
    LARS_PNG_INFO_APNG = 8,
    LARS_PNG_INFO_SUPPORTED = 9
};
enum {
    LARS_PNGD_OK = 0,
    LARS_PNGD_CRC = 1,           /* detail: IDAT chunk index */
    LARS_PNGD_ZLIB_HEADER = 2,   /* detail: CMF << 8 | FLG */
    LARS_PNGD_DEFLATE = 3,       /* detail: 1 block type, 2 stored length, 3 code lengths, 4 invalid code, 5 truncated */
    LARS_PNGD_FAR = 4,           /* a copy reaches before the stream start; detail: low 31 bits of the output position */
    LARS_PNGD_SHORT = 5,         /* too few decoded bytes; detail: min(decoded, 2^31 - 1) */
    LARS_PNGD_ADLER = 6,
    LARS_PNGD_FILTER = 7,        /* a filter byte above 4; detail: the row */
    LARS_PNGD_INTERNAL = 8       /* a bounded wait ran out or a table overflowed; detail: which */
};
int lars_png_info(const uint8_t *file, int64_t len, int64_t info[LARS_PNG_INFO_N], int64_t *idat_table, int64_t idat_cap);
size_t lars_png_decode_scratch_bytes(int64_t h, int64_t w, int channels, int64_t idat_bytes, int64_t idat_count);
int lars_d_decode_png_u8(const uint8_t *file, const int64_t *idat_table, int64_t idat_count, int64_t idat_bytes, int64_t h,
                         int64_t w, int channels, uint8_t *out, int32_t *status_dev, void *scratch, void *stream);
int lars_h_decode_png_u8(const uint8_t *file, int64_t len, uint8_t *out, size_t out_cap);
int lars_h_thumbnail_png_u8(const uint8_t *file, int64_t len, int fx, int fy, const int reduce_box[4], const float box[4],
                            int64_t new_h, int64_t new_w, int vertical_first, uint8_t *out);

/* The extended PNG decoder: every valid IHDR combination that is not APNG -- bit depths 1, 2, 4 and 16 and Adam7 interlace
 * besides the above -- as the array Pillow's np.asarray gives:
 *   colour type 0 (gray)     depth 1: one byte 0 / 1 per pixel (Pillow: bool); depth 2 / 4: uint8, sample x 85 / x 17;
 *                            depth 8: uint8; depth 16: native-endian uint16 (mode I;16; the file is big-endian)
 *   colour type 3 (palette)  uint8, the unscaled indices, whatever PLTE holds
 *   colour type 2 / 6        depth 16: uint8, the high byte of every sample
 *   colour type 4 (LA)       depth 8: [h][w][2]; depth 16: uint8 [h][w][4] = L, L, L, A of the high bytes (Pillow opens it as RGBA)
 * Interlace changes nothing in the result.  The zlib stream is decoded by the kernels of lars_d_decode_png_u8; the rows
 * of each pass are then unfiltered by a workgroup of their own and placed into the array.  An 8-bit file without
 * interlace takes lars_d_decode_png_u8's path unchanged.
 * lars_png_out_format: pure host code; channels and bytes per sample of that array for a (depth, colour type) pair.
 * lars_png_layout: pure host code; the filtered stream of a w x h picture: passes[k * LARS_PNGX_PASS_N + LARS_PNGX_PASS_*] for
 * each of the *npass non-empty passes (1 without interlace, up to 7 with; an Adam7 pass with no column or no row has no
 * bytes at all, not even filter bytes) and *need, the stream's length (saturating at INT64_MAX).
 * lars_png_decode_ex_scratch_bytes: device scratch of lars_d_decode_png_ex (0 for a picture it cannot decode: need must
 * stay below 2^31 and both sides within 2^24).
 * lars_d_decode_png_ex: as lars_d_decode_png_u8, with the IHDR numbers in place of channels; out holds h * w * channels *
 * itemsize bytes of lars_png_out_format.  A LARS_PNGD_FILTER detail is pass << 24 | row within the pass (pass 1 to 7, 0
 * without interlace).
 * lars_h_decode_png_ex, lars_h_thumbnail_png_ex: the host entry points; the thumbnail takes files whose array is uint8
 * L, RGB or RGBA (Pillow modes 1, I;16, P and LA are refused). */
#define LARS_PNGX_PASS_N 10
enum {                           /* positions in one pass of lars_png_layout's passes[] */
    LARS_PNGX_PASS_X0 = 0,       /* first column and row of the pass in the picture */
    LARS_PNGX_PASS_Y0 = 1,
    LARS_PNGX_PASS_DX = 2,       /* column and row step */
    LARS_PNGX_PASS_DY = 3,
    LARS_PNGX_PASS_W = 4,        /* columns and rows of the pass */
    LARS_PNGX_PASS_H = 5,
    LARS_PNGX_PASS_ROW_BYTES = 6,/* ceil(W * channels * depth / 8), without the filter byte */
    LARS_PNGX_PASS_OFFSET = 7,   /* of the pass's first filter byte in the stream */
    LARS_PNGX_PASS_BPP = 8,      /* filter distance max(1, channels * depth / 8) */
    LARS_PNGX_PASS_INDEX = 9     /* Adam7 pass number 1 to 7; 0 without interlace */
};
int lars_png_out_format(int depth, int color_type, int *channels, int *itemsize);
int lars_png_layout(int64_t w, int64_t h, int depth, int color_type, int interlace, int64_t passes[7 * LARS_PNGX_PASS_N],
                    int64_t *npass, int64_t *need);
size_t lars_png_decode_ex_scratch_bytes(int64_t h, int64_t w, int depth, int color_type, int interlace, int64_t idat_bytes,
                                        int64_t idat_count);
int lars_d_decode_png_ex(const uint8_t *file, const int64_t *idat_table, int64_t idat_count, int64_t idat_bytes, int64_t h,
                         int64_t w, int depth, int color_type, int interlace, uint8_t *out, int32_t *status_dev, void *scratch,
                         void *stream);
int lars_h_decode_png_ex(const uint8_t *file, int64_t len, uint8_t *out, size_t out_cap);
int lars_h_thumbnail_png_ex(const uint8_t *file, int64_t len, int fx, int fy, const int reduce_box[4], const float box[4],
                            int64_t new_h, int64_t new_w, int vertical_first, uint8_t *out);

/* Baseline JPEG files decoded on the device -- the same Image.open(io.BytesIO(img_bytes)) + np.array(img) of
 * load_image_from_db (process-images.py:181-193) for the format the cameras write, and the thumbnail after it.
 * Covered: SOF0 / SOF1 (Huffman, 8 bit), one interleaved scan, one component (L, [h][w]) or YCbCr at 4:4:4, 4:2:2 or 4:2:0
 * (RGB, [h][w][3]), restart intervals.  The pixels are libjpeg's JDCT_ISLOW ones with fancy upsampling: what Pillow's
 * np.asarray gives, bit for bit.  Damaged entropy data is an error here (Pillow pads it with grey).
 * lars_jpeg_info: pure host code.  Walks the marker segments of file[0..len), checks every length and table, and fills
 * info[LARS_JPEG_INFO_N] = { width, height, components, frame marker (0xC0 ...), precision, h0, v0, h1, v1, h2, v2 (sampling),
 * restart interval, entropy segment offset, entropy segment length, supported, LARS_JPEG_REASON_* }.
 * lars_jpeg_decode_scratch_bytes: device scratch of lars_d_decode_jpeg_u8 for that info (0 for what it cannot decode).
 * lars_d_decode_jpeg_u8: file_dev = the whole file on the device, head = its first info[LARS_JPEG_INFO_ENTROPY_OFFSET] bytes on the HOST (the tables are
 * read from there before the call returns), info as lars_jpeg_info gave it, out = h * w * components bytes on the device;
 * enqueues on stream and writes { LARS_JPGD_* status, detail } to the device int32 status_dev[2].
 * lars_h_decode_jpeg_u8: host file in, host pixels out (out_cap >= h * w * components); one upload, one download.
 * lars_h_thumbnail_jpeg_u8: host file in, lars_h_thumbnail_u8's plan numbers, host thumbnail out; the decoded pixels
 * never leave the device.  The decoder runs at full scale: the caller checks that Pillow's draft() would too (or calls
 * lars_h_thumbnail_jpeg_scaled_u8 below). */
#define LARS_JPEG_INFO_N 16
#define LARS_JPEG_INFO_SAMPLING_STRIDE 2   /* component c: info[LARS_JPEG_INFO_H0 + 2 c], info[LARS_JPEG_INFO_V0 + 2 c], c = 0, 1, 2 */
enum {                           /* positions in lars_jpeg_info's info[] */
    LARS_JPEG_INFO_WIDTH = 0,
    LARS_JPEG_INFO_HEIGHT = 1,
    LARS_JPEG_INFO_COMPONENTS = 2,
    LARS_JPEG_INFO_FRAME = 3,
    LARS_JPEG_INFO_PRECISION = 4,
    LARS_JPEG_INFO_H0 = 5,
    LARS_JPEG_INFO_V0 = 6,
    LARS_JPEG_INFO_RESTART_INTERVAL = 11,
    LARS_JPEG_INFO_ENTROPY_OFFSET = 12,
    LARS_JPEG_INFO_ENTROPY_BYTES = 13,
    LARS_JPEG_INFO_SUPPORTED = 14,
    LARS_JPEG_INFO_REASON = 15
};
enum {
    LARS_JPEG_REASON_NONE = 0,
    LARS_JPEG_REASON_PROGRESSIVE = 1,  /* SOF2 */
    LARS_JPEG_REASON_FRAME = 2,        /* lossless, arithmetic or hierarchical frame */
    LARS_JPEG_REASON_PRECISION = 3,    /* not 8 bit */
    LARS_JPEG_REASON_SCANS = 4,        /* more than one scan, or a scan that does not hold every component in order */
    LARS_JPEG_REASON_COMPONENTS = 5,   /* 2 or 4 components (CMYK / YCCK) */
    LARS_JPEG_REASON_COLORSPACE = 6,   /* RGB stored as such (Adobe transform 0, component ids R G B) */
    LARS_JPEG_REASON_SAMPLING = 7,     /* other than 4:4:4, 4:2:2, 4:2:0 */
    LARS_JPEG_REASON_DNL = 8,          /* height given by a DNL marker */
    LARS_JPEG_REASON_SIZE = 9          /* h * w * components >= 2^31 */
};
enum {
    LARS_JPGD_OK = 0,
    LARS_JPGD_RESTART = 1,       /* detail: restart markers found; one is missing, extra or out of sequence */
    LARS_JPGD_CODE = 2,          /* a bit pattern that is no code of the table in use; detail: the subsequence */
    LARS_JPGD_COEF = 3,          /* a coefficient index past 63; detail: the subsequence */
    LARS_JPGD_BLOCKS = 4,        /* the entropy data does not hold the frame's blocks; detail: blocks found (capped) */
    LARS_JPGD_INTERNAL = 5
};
int lars_jpeg_info(const uint8_t *file, int64_t len, int64_t info[LARS_JPEG_INFO_N]);
size_t lars_jpeg_decode_scratch_bytes(const int64_t info[LARS_JPEG_INFO_N]);
int lars_d_decode_jpeg_u8(const uint8_t *file_dev, const uint8_t *head, const int64_t info[LARS_JPEG_INFO_N], uint8_t *out,
                          int32_t *status_dev, void *scratch, void *stream);
int lars_h_decode_jpeg_u8(const uint8_t *file, int64_t len, uint8_t *out, size_t out_cap);
int lars_h_thumbnail_jpeg_u8(const uint8_t *file, int64_t len, int fx, int fy, const int reduce_box[4], const float box[4],
                             int64_t new_h, int64_t new_w, int vertical_first, uint8_t *out);

/* The same files decoded at 1/scale, scale = 1, 2, 4 or 8 (anything else: LARS_ERR_INVALID) -- what load_image_from_db(...,
 * thumbnail=True) really runs (process-images.py:186-189): img.thumbnail((400, 400)) calls draft(), and libjpeg decodes a
 * camera file at 1/2, 1/4 or 1/8.  The picture is ceil(h / scale) x ceil(w / scale); the pixels are libjpeg-turbo's for
 * scale_num / scale_denom = 1 / scale with JDCT_ISLOW and fancy upsampling, i.e. np.asarray(im) after im.draft() has set
 * im.decoderconfig == (scale, 0), bit for bit.  scale 1 gives the bytes of the functions above.
 * lars_jpeg_decode_scaled_scratch_bytes: device scratch of lars_d_decode_jpeg_scaled_u8 for that info and scale.
 * lars_d_decode_jpeg_scaled_u8: lars_d_decode_jpeg_u8 with out = ceil(h / scale) * ceil(w / scale) * components bytes.
 * lars_h_decode_jpeg_scaled_u8: host file in, host pixels of the scaled picture out.
 * lars_h_thumbnail_jpeg_scaled_u8: host file in, the plan numbers for the SCALED picture (box: the one draft() returns,
 * (0, 0, w / scale, h / scale), carried through the plan), host thumbnail out; the decoded pixels never leave the device. */
size_t lars_jpeg_decode_scaled_scratch_bytes(const int64_t info[LARS_JPEG_INFO_N], int scale);
int lars_d_decode_jpeg_scaled_u8(const uint8_t *file_dev, const uint8_t *head, const int64_t info[LARS_JPEG_INFO_N], int scale, uint8_t *out,
                                 int32_t *status_dev, void *scratch, void *stream);
int lars_h_decode_jpeg_scaled_u8(const uint8_t *file, int64_t len, int scale, uint8_t *out, size_t out_cap);
int lars_h_thumbnail_jpeg_scaled_u8(const uint8_t *file, int64_t len, int scale, int fx, int fy, const int reduce_box[4], const float box[4],
                                    int64_t new_h, int64_t new_w, int vertical_first, uint8_t *out);

/* Baseline JPEG files of 8-bit pictures, built on the device -- the Image.fromarray(corrected).save(save_path) that ends the
 * camera path (process-rgn.py:47 with :72-73; process-ndvi.py:114 reads the file back) and the img.save(buffer, format=img.format)
 * of an upload (process-images.py:247).  img is uint8 [h][w][channels]: 1 (L, one component) or 3 (RGB, stored as YCbCr);
 * quality 1..100; subsampling 0 = 4:4:4, 1 = 4:2:2, 2 = 4:2:0, Pillow's numbers (one channel: the data do not depend on it,
 * the sampling byte of the frame header does, as in Pillow's files); 1 <= h, w <= 65500 and h * w * channels < 2^31.  The file is byte for byte what Pillow on libjpeg-turbo writes with these arguments and its other
 * defaults: JFIF 1.01 header, the annex K tables scaled by the quality, the standard Huffman tables, one interleaved scan,
 * no restart markers.
 * lars_jpeg_bound: the largest file any picture of that shape can give at any quality (0 for a shape that cannot be
 * encoded): every block at its longest code per coefficient, every byte of that stuffed.  Pure host code.
 * lars_jpeg_header: pure host code.  The file's bytes up to and including SOS into out; returns their number, 0 (and the
 * error message set) for bad arguments or an out_cap that is too small (640 always suffices).
 * lars_jpeg_encode_scratch_bytes: device scratch of lars_d_encode_jpeg_u8 (0 for a shape that cannot be encoded).
 * lars_d_encode_jpeg_u8: device img / out (out_cap >= lars_jpeg_bound) / scratch; enqueues on stream and writes the file's
 * length to the device int64 *out_len_dev (0: a buffer overflowed, which the bound rules out).
 * lars_h_encode_jpeg_u8: host img / out; one upload, then the length, then out_len bytes into out. */
size_t lars_jpeg_bound(int64_t h, int64_t w, int channels, int subsampling);
int64_t lars_jpeg_header(int64_t h, int64_t w, int channels, int subsampling, int quality, uint8_t *out, size_t out_cap);
size_t lars_jpeg_encode_scratch_bytes(int64_t h, int64_t w, int channels, int subsampling);
int lars_d_encode_jpeg_u8(const uint8_t *img, int64_t h, int64_t w, int channels, int quality, int subsampling, uint8_t *out,
                          size_t out_cap, int64_t *out_len_dev, void *scratch, void *stream);
int lars_h_encode_jpeg_u8(const uint8_t *img, int64_t h, int64_t w, int channels, int quality, int subsampling, uint8_t *out,
                          size_t out_cap, int64_t *out_len);

/* ------------------------------------------------------------------ image files (host only, no GPU work) */
/* TIFF 6.0 LZW (compression 5, MSB-first codes, early width change) of one strip / tile: decodes at most ndst bytes
 * into dst, *nout = bytes produced.  For lars_image_processing_amd/tiffio.py, which reads the multi-sample 16-bit
 * TIFFs that PIL.Image.open (backend-process.py:52) reduces to 8 bits. */
int lars_h_tiff_lzw_decode(const uint8_t *src, int64_t nsrc, uint8_t *dst, int64_t ndst, int64_t *nout);
/* Every strip / tile of an image in one call, shared by `threads` workers: chunk i = file[offsets[i], +counts[i])
 * decodes into dst + i * chunk_bytes (at most chunk_bytes bytes), produced[i] = bytes that came out. */
int lars_h_tiff_lzw_decode_chunks(const uint8_t *file, int64_t file_len, const uint64_t *offsets, const uint64_t *counts,
                                  int64_t nchunks, uint8_t *dst, int64_t chunk_bytes, int64_t *produced, int threads);

/* TIFF files decoded on the device -- the Image.open(io.BytesIO(...)) of an upload (process-images.py:183, :228) for the first
 * of the accepted extensions (process-images.py:1237, backend-process.py:88) and the format the reference writes itself
 * (backend-process.py:57), plus the thumbnail after it (process-images.py:186-189).
 * Covered: classic TIFF, first directory, either byte order, 8 or 16 bit unsigned samples (equal across samples), no
 * compression or LZW, predictor 1 or 2, chunky or planar, strips or tiles.  The pixels come out as tiffio.read_tiff gives
 * them: [h][w][samples] ([h][w] for one sample), uint8 or native-endian uint16.
 * Float32 samples as well (BitsPerSample 32 with SampleFormat 3 for every sample, the type of the index planes): the same
 * layouts and compressions with predictor 1, 2 (differencing of the 32-bit patterns modulo 2^32) or 3 (the floating-point
 * predictor, libtiff's fpAcc: per row of a strip / tile, padding columns included, the running sum with the stride of a
 * pixel's samples over four byte planes, most significant first in either byte order).  Native floats come out, bit for
 * bit, whatever the file's byte order.  info[LARS_TIFF_INFO_BITS] == 32 means float32: no other 32-bit kind is decoded.
 * lars_tiff_info: pure host code.  Walks the first directory of file[0..len) by read_tiff's rules, checks every offset and
 * count against len, and fills info[LARS_TIFF_INFO_N] (positions below); chunk_table (may be NULL with table_cap 0)
 * receives { offset, byte count } of the first table_cap strips / tiles.  A valid file the device does not decode has
 * supported 0 and a LARS_TIFF_REASON_*; structural damage is LARS_ERR_INVALID.
 * lars_h_decode_tiff: host file in, host samples out (out_cap in BYTES >= h * w * samples * bits / 8); one upload, one download.
 * lars_h_thumbnail_tiff_u8: host file in (8 bit, one BlackIsZero sample or RGB, no extra samples), lars_h_thumbnail_u8's
 * plan numbers, host thumbnail out; the decoded pixels never leave the device.
 * lars_tiff_info_deflate, lars_h_decode_tiff_deflate, lars_h_thumbnail_tiff_deflate_u8: the same three for callers who opt in
 * to Deflate on the device -- compression 8 (GDAL's COMPRESS=DEFLATE, tifffile, Pillow's tiff_adobe_deflate) and 32946, the
 * files the uploads of process-images.py:1237 and backend-process.py:52, :88 most often are.  The walk treats such a file as
 * it treats an LZW file (geometry, chunk table, predictor 1 / 2, the 2^31 limit on the padded chunks) and ends with
 * supported 1; for every other file each gives what its sibling gives.  Every strip / tile is one zlib stream, judged as
 * tiffio._chunk judges it: LARS_TIFD_CORRUPT, LARS_TIFD_PAST and LARS_TIFD_SHORT for the first such chunk in file order. */
#define LARS_TIFF_INFO_N 16
enum {                           /* positions in lars_tiff_info's info[] */
    LARS_TIFF_INFO_WIDTH = 0,
    LARS_TIFF_INFO_HEIGHT = 1,
    LARS_TIFF_INFO_SAMPLES = 2,
    LARS_TIFF_INFO_BITS = 3,
    LARS_TIFF_INFO_COMPRESSION = 4,
    LARS_TIFF_INFO_PREDICTOR = 5,
    LARS_TIFF_INFO_PLANAR = 6,
    LARS_TIFF_INFO_BIG_ENDIAN = 7,
    LARS_TIFF_INFO_PHOTOMETRIC = 8,   /* -1: the tag is missing */
    LARS_TIFF_INFO_EXTRA_SAMPLES = 9,
    LARS_TIFF_INFO_TILED = 10,
    LARS_TIFF_INFO_CHUNK_W = 11,
    LARS_TIFF_INFO_CHUNK_H = 12,
    LARS_TIFF_INFO_CHUNKS = 13,
    LARS_TIFF_INFO_SUPPORTED = 14,
    LARS_TIFF_INFO_REASON = 15
};
enum {
    LARS_TIFF_REASON_NONE = 0,
    LARS_TIFF_REASON_BIGTIFF = 1,        /* 64-bit offsets (magic 43) */
    LARS_TIFF_REASON_BITS = 2,           /* samples that are not all 8, all 16 or all 32 bits wide */
    LARS_TIFF_REASON_SAMPLE_FORMAT = 3,  /* signed samples, floats of 8 or 16 bits, integers of 32 */
    LARS_TIFF_REASON_DEFLATE = 4,        /* compression 8 / 32946 (tiffio.read_tiff reads them) */
    LARS_TIFF_REASON_PACKBITS = 5,
    LARS_TIFF_REASON_JPEG = 6,           /* compression 6 / 7 */
    LARS_TIFF_REASON_CCITT = 7,          /* compression 2, 3, 4 */
    LARS_TIFF_REASON_COMPRESSION = 8,    /* any other scheme */
    LARS_TIFF_REASON_PREDICTOR = 9,      /* other than 1 and 2, or 3 without float32 samples */
    LARS_TIFF_REASON_OLD_LZW = 10,       /* a strip in the old bit order (LSB first), which lars_h_tiff_lzw_decode refuses too */
    LARS_TIFF_REASON_SIZE = 11           /* 2^31 or more decoded bytes (tile padding included) */
};
enum {
    LARS_TIFD_OK = 0,
    LARS_TIFD_CORRUPT = 1,       /* an LZW code the table does not hold; detail: the strip / tile */
    LARS_TIFD_SHORT = 2,         /* a strip / tile decodes to too few bytes; detail: the strip / tile */
    LARS_TIFD_PAST = 3           /* a Deflate strip / tile goes on behind the bytes the directory gives it; detail: the strip / tile */
};
int lars_tiff_info(const uint8_t *file, int64_t len, int64_t info[LARS_TIFF_INFO_N], int64_t *chunk_table, int64_t table_cap);
int lars_h_decode_tiff(const uint8_t *file, int64_t len, void *out, size_t out_cap);
int lars_tiff_info_deflate(const uint8_t *file, int64_t len, int64_t info[LARS_TIFF_INFO_N], int64_t *chunk_table, int64_t table_cap);
int lars_h_decode_tiff_deflate(const uint8_t *file, int64_t len, void *out, size_t out_cap);
int lars_h_thumbnail_tiff_deflate_u8(const uint8_t *file, int64_t len, int fx, int fy, const int reduce_box[4], const float box[4],
                                     int64_t new_h, int64_t new_w, int vertical_first, uint8_t *out);
int lars_h_thumbnail_tiff_u8(const uint8_t *file, int64_t len, int fx, int fy, const int reduce_box[4], const float box[4],
                             int64_t new_h, int64_t new_w, int vertical_first, uint8_t *out);

/* LZW TIFF files built on the device -- the Image.fromarray(corrected).save(".../<name>_wb.tif") of the batch job
 * (backend-process.py:57) and the lut_format="tiff" pictures of the directory driver.  img is [h][w][channels] of uint8
 * (itemsize 1) or native-endian uint16 (itemsize 2), channels 1..5.  The file is a classic little-endian TIFF: strips of
 * rows_per_strip rows, chunky samples, Compression 5, Predictor 2 (horizontal differencing per sample modulo 2^bits, every
 * row on its own) when predictor is not 0; strip data first, every strip on an even offset, then the directory with the tags
 * and values of tiffio.write_tiff.  rows_per_strip 0: the largest row count whose uncompressed strip stays within the tuning
 * knob tiff_strip_bytes (lars_set_tuning: 1 .. 1073741824, default 65536; at least one row); the files do depend on it.
 * Every strip is the stream of the greedy encoder: the longest match in the table at every step, a Clear code when the
 * table holds 4094 codes, a leading Clear, a trailing EndOfInformation, codes MSB first at TIFF's widths -- libtiff's bytes.
 * lars_tiff_bound: pure host code.  The largest file any picture of that shape can give (0 for a shape that cannot be
 * encoded): every input byte at most one 12-bit code, one Clear per 3836 codes, the leading Clear and EndOfInformation, one
 * pad byte per strip, the header and the directory with its arrays.
 * lars_tiff_encode_scratch_bytes: device scratch of lars_d_encode_tiff (0 for a shape that cannot be encoded).
 * lars_d_encode_tiff: device img / out (both on even addresses) / scratch; enqueues on stream.  status_dev: two device ints,
 * { LARS_TIFE_*, detail }; out_len_dev: the file's length, also under LARS_TIFE_NOSPACE (what out_cap would have had to be),
 * where nothing of out is valid.  Any out_cap is taken; lars_tiff_bound always suffices.
 * lars_h_encode_tiff: host img / out; one upload, then the status and the length, then out_len bytes into out. */
enum {
    LARS_TIFE_OK = 0,
    LARS_TIFE_NOSPACE = 1,       /* the file is longer than out_cap; detail: 0 */
    LARS_TIFE_TOO_LARGE = 2,     /* the file would reach 4 GiB; detail: 0 */
    LARS_TIFE_OVERFLOW = 3       /* a strip outgrew its buffer, which the bound rules out; detail: the strip */
};
size_t lars_tiff_bound(int64_t h, int64_t w, int channels, int itemsize, int64_t rows_per_strip);
size_t lars_tiff_encode_scratch_bytes(int64_t h, int64_t w, int channels, int itemsize, int64_t rows_per_strip);
int lars_d_encode_tiff(const void *img, int64_t h, int64_t w, int channels, int itemsize, int64_t rows_per_strip, int predictor,
                       uint8_t *out, size_t out_cap, int64_t *out_len_dev, int32_t *status_dev, void *scratch, void *stream);
int lars_h_encode_tiff(const void *img, int64_t h, int64_t w, int channels, int itemsize, int64_t rows_per_strip, int predictor,
                       uint8_t *out, size_t out_cap, int64_t *out_len);
/* The same four for float32 samples -- the index planes themselves (NDVI, GNDVI, NDWI), losslessly, as the single-band float
 * TIFF that GDAL, rasterio and QGIS exchange them in.  img is [h][w][channels] of native float32, channels 1..5.  The file is
 * the one above with BitsPerSample 32 and SampleFormat 3 per sample and the directory of tiffio.write_float_tiff; predictor
 * 0 writes no Predictor tag, any other value Predictor 3 (libtiff's fpDiff: every row as four planes of w * channels bytes,
 * plane 0 the most significant byte of every sample, each byte minus the byte `channels` positions earlier, across the plane
 * borders).  Strips, the knob, the streams (libtiff's bytes), the bound's derivation (a row has w * channels * 4 bytes),
 * status_dev and LARS_TIFE_* are those of the integer entry points, which go on refusing itemsize 4. */
size_t lars_tiff_f32_bound(int64_t h, int64_t w, int channels, int64_t rows_per_strip);
size_t lars_tiff_f32_encode_scratch_bytes(int64_t h, int64_t w, int channels, int64_t rows_per_strip);
int lars_d_encode_tiff_f32(const float *img, int64_t h, int64_t w, int channels, int64_t rows_per_strip, int predictor, uint8_t *out,
                           size_t out_cap, int64_t *out_len_dev, int32_t *status_dev, void *scratch, void *stream);
int lars_h_encode_tiff_f32(const float *img, int64_t h, int64_t w, int channels, int64_t rows_per_strip, int predictor, uint8_t *out,
                           size_t out_cap, int64_t *out_len);
/* lars_h_process_image with every requested index plane also encoded as a float32 TIFF on the device
 * (lars_d_encode_tiff_f32, one sample, predictor and rows_per_strip as there): the plane an index file holds never crosses
 * PCIe as 4 bytes per pixel, only its LZW file does.  out_tiff[k] (host, tiff_cap bytes, at least lars_tiff_f32_bound(h, w, 1,
 * rows_per_strip)) is needed for every index in index_mask; tiff_len[k] receives the file's length.  out_index, out_rgba and
 * cmap_lut as in lars_h_process_image; each may be NULL. */
int lars_h_process_image_tiff_f32(const void *img, int64_t h, int64_t w, int channels, int dtype,
                                  int apply_wb, uint32_t index_mask, int want_hist,
                                  uint8_t *out_wb, float *const out_index[3],
                                  lars_stats *stats /* [3] */, float *medians /* [3][2] */,
                                  uint8_t *const out_rgba[3], const uint8_t *const cmap_lut[3],
                                  int predictor, int64_t rows_per_strip,
                                  uint8_t *const out_tiff[3], size_t tiff_cap, int64_t tiff_len[3]);
/* Deflate TIFF files built on the device: the entry points above with Compression 8 (GDAL's COMPRESS=DEFLATE, the usual choice
 * with a predictor for float rasters).  Arguments, strips, the knob tiff_strip_bytes, the directory (tiffio.write_tiff(...,
 * deflate=True) / write_float_tiff(..., deflate=True) for the same array, rows_per_strip and predictor), status_dev, LARS_TIFE_*
 * and the 4 GiB refusal are those of the LZW entry points; only the strips' streams differ, and they are coded in parallel: one
 * workgroup per 32768 stored bytes of a strip.  The stream of a strip of n stored bytes (after the predictor, little-endian):
 * 78 01; for every part of 32768 bytes (the last may be shorter) one block -- dynamic Huffman over literals only (zlib's
 * Z_HUFFMAN_ONLY), or stored where that is not shorter; behind a dynamic block that is not the strip's last an empty stored
 * block (00 00 FF FF after three zero bits and the padding), so that every part ends on a byte boundary; BFINAL on the last;
 * the Adler-32 of the n bytes.  A function of the strip's bytes alone; any inflate reads it (lars_h_decode_tiff_deflate too).
 * With the knob deflate_matching at 1 (lars_set_tuning: 0 or 1, default 0) a part whose block of literals and length / distance
 * pairs (matches within the part only, tests/deflate_lz_model.py) is shorter than both other forms is written as that block;
 * every other part, the framing and the bounds are as at 0.
 * lars_tiff_deflate_bound: pure host code; per strip 2 header bytes, its n bytes, 5 bytes per part (a stored block's header;
 * a dynamic block with its flush is only chosen where it is no longer), 4 checksum bytes and one pad byte, then the header and
 * the directory with its arrays as in lars_tiff_bound; 0 for a shape that cannot be encoded.
 * lars_tiff_deflate_encode_scratch_bytes: device scratch of lars_d_encode_tiff_deflate (about twice the picture: the staged
 * predictor output and one slot per part). */
size_t lars_tiff_deflate_bound(int64_t h, int64_t w, int channels, int itemsize, int64_t rows_per_strip);
size_t lars_tiff_deflate_encode_scratch_bytes(int64_t h, int64_t w, int channels, int itemsize, int64_t rows_per_strip);
int lars_d_encode_tiff_deflate(const void *img, int64_t h, int64_t w, int channels, int itemsize, int64_t rows_per_strip, int predictor,
                               uint8_t *out, size_t out_cap, int64_t *out_len_dev, int32_t *status_dev, void *scratch, void *stream);
int lars_h_encode_tiff_deflate(const void *img, int64_t h, int64_t w, int channels, int itemsize, int64_t rows_per_strip, int predictor,
                               uint8_t *out, size_t out_cap, int64_t *out_len);
/* ... and for float32 samples (Predictor 3 when predictor is not 0), as lars_*_encode_tiff_f32 */
size_t lars_tiff_float32_deflate_bound(int64_t h, int64_t w, int channels, int64_t rows_per_strip);
size_t lars_tiff_float32_deflate_encode_scratch_bytes(int64_t h, int64_t w, int channels, int64_t rows_per_strip);
int lars_d_encode_tiff_deflate_float32(const float *img, int64_t h, int64_t w, int channels, int64_t rows_per_strip, int predictor, uint8_t *out,
                                   size_t out_cap, int64_t *out_len_dev, int32_t *status_dev, void *scratch, void *stream);
int lars_h_encode_tiff_deflate_float32(const float *img, int64_t h, int64_t w, int channels, int64_t rows_per_strip, int predictor, uint8_t *out,
                                   size_t out_cap, int64_t *out_len);
/* lars_h_process_image_tiff_f32 with the compression named: 5 (LZW, the same call) or 8 (Deflate: lars_d_encode_tiff_deflate_float32,
 * tiff_cap at least lars_tiff_float32_deflate_bound(h, w, 1, rows_per_strip)); any other value is LARS_ERR_INVALID. */
int lars_h_process_image_tiff_float32(const void *img, int64_t h, int64_t w, int channels, int dtype,
                                              int apply_wb, uint32_t index_mask, int want_hist,
                                              uint8_t *out_wb, float *const out_index[3],
                                              lars_stats *stats /* [3] */, float *medians /* [3][2] */,
                                              uint8_t *const out_rgba[3], const uint8_t *const cmap_lut[3],
                                              int compression, int predictor, int64_t rows_per_strip,
                                              uint8_t *const out_tiff[3], size_t tiff_cap, int64_t tiff_len[3]);

/* ------------------------------------------------- nodata-aware processing (csrc/masked.hip) */
/* The per-pixel path for pictures that are not picture everywhere: an orthomosaic's transparent or black frame, the reflected
 * border align_images leaves, a plot cut out with a mask.  With V the valid pixels in raster order, every result is the
 * reference's on the image img[valid][None, :, :] of shape [1][|V|][channels], scattered back:
 *   np.percentile(ch, (2, 98)) of fix_white_balance     process-images.py:437      over the valid samples only
 *   corrected image                                     process-images.py:438-441  0 in every channel outside
 *   calculate_index                                     process-images.py:449-490  float32 NaN 0x7FC00000 outside
 *   analyze_index, plt.hist(bins=50, range=(-1, 1))     process-images.py:492-513, process-ndvi.py:97
 *                                                       of the valid values; coverage relative to |V| (numpy.ma's rules)
 *   imshow(cmap, vmin=-1, vmax=1)                       process-images.py:695      (0, 0, 0, 0) outside: Colormap.set_bad's default
 *
 * lars_d_valid_mask: which pixels count, one byte each (1 = valid, 0 = not; [npix] uint8 in raster order, no bit packing),
 * and their number.  A pixel is valid where user_valid (device, [npix] uint8, nonzero = allowed; NULL = all; may be out_mask
 * itself) allows it AND, with use_alpha, its channel 3 is nonzero (channels >= 4) AND, with has_nodata, its R, G and NIR samples
 * are not all equal to nodata.  uint8 / uint16 samples, channels >= 3.  *count_dev (device uint64) is zeroed by the call and
 * receives |V|: a wave reduction, then one atomic per workgroup.  Masks 4-byte, count_dev 8-byte aligned.
 * lars_d_masked_channel_hist: lars_d_channel_hist of one image over the valid pixels only -- hist [3][256] (LARS_U8: private
 * copies in LDS) or [3][65536] (LARS_U16: global atomics) uint32, zeroed by the call.  lars_d_wb_table(hist, 1, |V|, ...)
 * then gives the percentiles and the table, the degenerate p98 == p2 channel and the uint16 threshold form included.
 * lars_d_masked_fused: lars_d_fused for one image (a->ntiles == 1) under a mask.  Outside the mask out_wb is 0, out_index
 * NaN, out_rgba (0, 0, 0, 0).  a->stats must be NULL and a->flags 0: instead compact[k] (device, room for npix float32; NULL
 * = not wanted; compact itself may be NULL) receives the valid values of index k in any order -- every wave takes its slots
 * from *cursor_dev (device uint64, zeroed by the call, |V| afterwards) with one atomic -- and lars_d_array_stats_f32 /
 * lars_d_median_pair_f32 over those |V| values give the record and the median.  out_rgba[k] needs cmap_lut[k].  Planes and
 * out_wb 16-byte aligned. */
int lars_d_valid_mask(const void *img, int64_t npix, int channels, int dtype, const uint8_t *user_valid, int use_alpha,
                      int has_nodata, int nodata, uint8_t *out_mask, uint64_t *count_dev, void *stream);
int lars_d_masked_channel_hist(const void *img, int64_t npix, int channels, int dtype, const uint8_t *valid,
                               uint32_t *hist, void *stream);
int lars_d_masked_fused(const lars_fused_args *a, const uint8_t *valid, float *const compact[3], uint64_t *cursor_dev);
/* valid_mask(img_array, nodata, alpha): lars_d_valid_mask of a host image; out_mask is host [h][w] uint8. */
int lars_h_valid_mask(const void *img, int64_t h, int64_t w, int channels, int dtype, int use_alpha, int has_nodata, int nodata,
                      uint8_t *out_mask, int64_t *valid_pixels /* may be NULL */);
/* lars_h_process_image under a mask, and its file-writing twins in one call.  valid: host [h][w] uint8, nonzero = valid, or
 * NULL; use_alpha / has_nodata / nodata as above; the three rules combine with AND.  *valid_pixels receives |V|; with
 * |V| == 0 the call fails with LARS_ERR_INVALID ("no valid pixel") and *valid_pixels is 0 (-1 after any earlier failure).
 * file_kind 0: no files, out_rgba[k] with cmap_lut[k] receives the RGBA picture.  file_kind 1: lars_h_process_image_png's
 * RGBA files (png_mode 1; a transparent frame).  file_kind 5 / 8: lars_h_process_image_tiff_float32's LZW / Deflate files
 * of the planes (NaN outside) with predictor and rows_per_strip.  out_file[k] (host, file_cap bytes: at least that call's
 * bound) and file_len[k] as there.  Colormap entry planes and palette PNGs are refused: the 256-entry palette has no
 * free entry for "no data".  Statistics, histogram and medians are those of the valid values; everything else as in
 * lars_h_process_image. */
int lars_h_process_image_masked(const void *img, int64_t h, int64_t w, int channels, int dtype,
                                int apply_wb, uint32_t index_mask, int want_hist,
                                uint8_t *out_wb, float *const out_index[3],
                                lars_stats *stats /* [3] */, float *medians /* [3][2] */,
                                uint8_t *const out_rgba[3], const uint8_t *const cmap_lut[3],
                                const uint8_t *valid, int use_alpha, int has_nodata, int nodata, int64_t *valid_pixels,
                                int file_kind, int predictor, int64_t rows_per_strip,
                                uint8_t *const out_file[3], size_t file_cap, int64_t file_len[3]);

/* ------------------------------------------------- zonal statistics (csrc/zonal.hip) */
/* One record per plot.  zones is an [npix] raster of labels 0 .. nzones in raster order, zone_bytes wide: 1 (uint8), 2 (uint16)
 * or 4 (int32); label 0 is "in no zone"; nzones is 1 .. LARS_ZONES_MAX.  valid is lars_d_valid_mask's byte mask or NULL (every
 * pixel counts).  With S_z = x[valid & (zones == z)], zone z's record and median pair are lars_d_array_stats_f32's and
 * lars_d_median_pair_f32's of S_z (analyze_index on each plot, process-images.py:492-513; plt.hist, process-ndvi.py:97): count =
 * |S_z|, coverage relative to it, NaN samples counted in nans as there.  An empty zone has count 0 and a NaN pair.  Everything
 * is bit-reproducible except sum / sumsq: the values of a zone are added in the order the scatter placed them.
 *
 * lars_d_zone_count: counts_dev[nzones + 1] (device uint64, zeroed by the call) receives |S_z| at z, and at 0 the pixels with
 * label 0 or outside valid; *bad_dev (device uint64, zeroed by the call) the labels below 0 or above nzones, which are counted
 * nowhere else.  Waves aggregate equal labels with ballots before they add: one atomic per run of a label, not per pixel.
 * lars_d_zone_offsets: offsets_dev[nzones + 1] (device uint64) receives the segment ends -- offsets[0] = 0, offsets[z] =
 * counts[1] + .. + counts[z]: zone z owns the slots offsets[z - 1] .. offsets[z] - 1 -- and cursors_dev[nzones + 1] zeros.
 * lars_d_zone_scatter: for every index k of index_mask, out[k] (device, room for offsets[nzones] float32) receives planes[k]'s
 * values zone by zone: out[k][offsets[z - 1] ..] holds S_z in any order.  The indices share the slots (one cursor per zone,
 * zeroed by the call).  zones, valid and nzones must be those the counts were taken from; a slot outside its segment is not
 * written.
 * lars_d_zone_stats: stats_dev[nzones] and medians_dev[nzones][2] (entry z - 1 for zone z) from one plane's scattered values,
 * one workgroup per zone.  Zones with more than split_pixels values are left untouched: the caller runs
 * lars_d_array_stats_f32 / lars_d_median_pair_f32 on values + offsets[z - 1] for them, as lars_h_zonal_stats_f32 does with
 * the knob zone_split_pixels (lars_set_tuning: 64 .. 1073741824, default 131072; results never depend on it). */
#define LARS_ZONES_MAX 65535
int lars_d_zone_count(const void *zones, int zone_bytes, const uint8_t *valid, int64_t npix, int64_t nzones,
                      uint64_t *counts_dev, uint64_t *bad_dev, void *stream);
int lars_d_zone_offsets(const uint64_t *counts_dev, int64_t nzones, uint64_t *offsets_dev, uint64_t *cursors_dev, void *stream);
int lars_d_zone_scatter(const float *const planes[3], uint32_t index_mask, const void *zones, int zone_bytes, const uint8_t *valid,
                        int64_t npix, int64_t nzones, const uint64_t *offsets_dev, uint64_t *cursors_dev, float *const out[3],
                        void *stream);
int lars_d_zone_stats(const float *values, const uint64_t *offsets_dev, const uint64_t *counts_dev, int64_t nzones, float threshold,
                      int want_hist, int64_t split_pixels, lars_stats *stats_dev /* [nzones] */, float *medians_dev /* [nzones][2] */,
                      void *stream);
/* zonal_statistics(index_array, zones, ...): the four stages on a host float32 [h][w] plane -- one upload, one download.
 * valid: host [h][w] uint8, nonzero = counts, or NULL.  stats[nzones] and medians[nzones][2] are host arrays.  Labels
 * outside 0 .. nzones: LARS_ERR_INVALID with their number in *bad_labels (0 on success, -1 after any earlier failure). */
int lars_h_zonal_stats_f32(const float *x, const void *zones, int zone_bytes, const uint8_t *valid /* may be NULL */, int64_t h, int64_t w,
                           int64_t nzones, float threshold, int want_hist, lars_stats *stats /* [nzones] */,
                           float *medians /* [nzones][2] */, int64_t *bad_labels);
/* process_image_zones: lars_h_process_image_masked without files (its file_kind 0) plus one record per zone and index.  The
 * picture-level results -- percentiles, corrected image, planes, pictures, stats, medians, *valid_pixels -- are that call's
 * with the same valid / use_alpha / has_nodata / nodata: zones do not change which pixels the white balance sees.  zones:
 * host [h][w] labels as above.  zone_stats[3][nzones] and zone_medians[3][nzones][2] (host; rows of indices outside
 * index_mask untouched) describe S_z = plane[valid & (zones == z)] with the coverage thresholds of the picture-level
 * records.  Bad labels as in lars_h_zonal_stats_f32.  index_mask must not be empty. */
int lars_h_process_image_zones(const void *img, int64_t h, int64_t w, int channels, int dtype,
                               int apply_wb, uint32_t index_mask, int want_hist,
                               uint8_t *out_wb, float *const out_index[3],
                               lars_stats *stats /* [3] */, float *medians /* [3][2] */,
                               uint8_t *const out_rgba[3], const uint8_t *const cmap_lut[3],
                               const uint8_t *valid, int use_alpha, int has_nodata, int nodata, int64_t *valid_pixels,
                               const void *zones, int zone_bytes, int64_t nzones,
                               lars_stats *zone_stats /* [3][nzones] */, float *zone_medians /* [3][nzones][2] */,
                               int64_t *bad_labels);

/* ------------------------------------------------- zones from polygons (csrc/zone_raster.hip) */
/* The label raster of the zone stages, made on the device from plot outlines: analyze_index per plot (process-images.py:492-513)
 * for callers who hold the outlines of their plots and no raster.
 *
 * The polygons.  verts is double [nverts][2], (x, y) in pixel units: x along the columns, y along the rows, pixel (row i, column j)
 * has the centre cx = j + 0.5, cy = i + 0.5.  Ring r has the vertices ring_starts[r] .. ring_starts[r + 1] - 1 (three or more,
 * closed implicitly; a first vertex repeated at the end makes a zero-length edge, which counts for nothing); polygon k has the
 * rings poly_starts[k] .. poly_starts[k + 1] - 1 (one or more).  ring_starts[nrings + 1] and poly_starts[npolys + 1] are int32,
 * start at 0, rise, and end at nverts and nrings.  The edges of all rings of a polygon are pooled: holes and parts need no other
 * rule.  1 <= npolys <= LARS_ZONES_MAX, nverts <= LARS_ZONE_VERTS_MAX, every coordinate finite with |v| <= 1e9.
 *
 * The rule, in IEEE float64 with every operation rounded once.  An edge (x0, y0) - (x1, y1) with y0 == y1 crosses no row.
 * Otherwise (xa, ya) is its end with the smaller y and (xb, yb) the other; it crosses row i iff ya <= cy < yb, at
 *     xc = xa + ((cy - ya) * (xb - xa)) / (yb - ya)                     evaluated in exactly this order,
 * so an edge two plots share crosses at the same xc for both, whichever way their rings run.  Pixel (i, j) is inside a polygon iff
 * the number of its crossings of row i with xc <= cx is odd (even-odd, half-open on both axes).  Polygon k labels its pixels k + 1;
 * a pixel inside several takes the largest label (the later polygon wins, as painting in order would), a pixel inside none is 0.
 * A polygon that covers no pixel centre is an empty zone.  The result is this definition bit for bit on every run.
 *
 * lars_d_zone_rasterize: all three arrays and labels[h][w] (int32, zeroed by the call) on the device; scratch:
 * lars_zone_rasterize_scratch_bytes(npolys) bytes, 256-byte aligned; verts 16-byte aligned.  The arrays are not checked on the device: indices that
 * leave them are clamped, so arrays that break the rules above give wrong labels and no access outside the buffers.  The labels
 * feed lars_d_zone_count / lars_d_zone_scatter as they are, with zone_bytes 4 and nzones = npolys.
 * lars_d_zone_labels_narrow: out[npix] uint8 (zone_bytes 1) or uint16 (2) = the int32 labels, for a raster that goes to the host. */
#define LARS_ZONE_VERTS_MAX 16777216
size_t lars_zone_rasterize_scratch_bytes(int64_t npolys);
int lars_d_zone_rasterize(const double *verts, int64_t nverts, const int32_t *ring_starts, int64_t nrings, const int32_t *poly_starts,
                          int64_t npolys, int64_t h, int64_t w, int32_t *labels, void *scratch, void *stream);
int lars_d_zone_labels_narrow(const int32_t *labels, int64_t npix, int zone_bytes, void *out, void *stream);
/* rasterize_zones(polygons, shape): host arrays in (checked: the rules above, LARS_ERR_INVALID names the first ring or vertex that
 * breaks them), host labels[h][w] out, zone_bytes 1, 2 or 4 wide; npolys must fit the width (255, 65535). */
int lars_h_rasterize_zones(const double *verts, int64_t nverts, const int32_t *ring_starts, int64_t nrings, const int32_t *poly_starts,
                           int64_t npolys, int64_t h, int64_t w, int zone_bytes, void *labels);
/* lars_h_zonal_stats_f32 with the labels rasterised on the device from host polygon arrays instead of uploaded: nzones = npolys,
 * stats[npolys], medians[npolys][2].  labels_out: NULL (the labels never leave the device) or host [h][w] labels, label_bytes 1,
 * 2 or 4 wide.  By definition the records are those of lars_h_zonal_stats_f32 on lars_h_rasterize_zones's raster. */
int lars_h_zonal_stats_polygons_f32(const float *x, const double *verts, int64_t nverts, const int32_t *ring_starts, int64_t nrings,
                                    const int32_t *poly_starts, int64_t npolys, const uint8_t *valid /* may be NULL */, int64_t h, int64_t w,
                                    float threshold, int want_hist, lars_stats *stats /* [npolys] */, float *medians /* [npolys][2] */,
                                    void *labels_out /* may be NULL */, int label_bytes);
/* lars_h_process_image_zones likewise: zone_stats[3][npolys], zone_medians[3][npolys][2]. */
int lars_h_process_image_zones_polygons(const void *img, int64_t h, int64_t w, int channels, int dtype,
                                        int apply_wb, uint32_t index_mask, int want_hist,
                                        uint8_t *out_wb, float *const out_index[3],
                                        lars_stats *stats /* [3] */, float *medians /* [3][2] */,
                                        uint8_t *const out_rgba[3], const uint8_t *const cmap_lut[3],
                                        const uint8_t *valid, int use_alpha, int has_nodata, int nodata, int64_t *valid_pixels,
                                        const double *verts, int64_t nverts, const int32_t *ring_starts, int64_t nrings,
                                        const int32_t *poly_starts, int64_t npolys,
                                        lars_stats *zone_stats /* [3][npolys] */, float *zone_medians /* [3][npolys][2] */,
                                        void *labels_out /* may be NULL */, int label_bytes);

/* ------------------------------------------------- zones from regions (csrc/regions.hip) */
/* The label raster of the zone stages, made on the device from the picture itself: the connected regions of a foreground mask
 * (canopy patches, gaps, wet spots), for callers who hold no outlines at all.
 *
 * The definition.  mask is uint8 [h][w], nonzero = foreground; 1 <= h, w and h * w < 2^31.  Two foreground pixels are neighbours
 * when they share an edge (connectivity 4) or an edge or a corner (connectivity 8).  A region is a maximal connected set of
 * foreground pixels.  Regions are numbered 1 .. R in raster order of their first pixel, the one with the smallest flat index
 * y * w + x (scipy.ndimage.label's numbering with the cross / the full 3 x 3 structure).  With min_pixels > 1 the regions of fewer
 * pixels become 0 and the others are numbered 1 .. R in the same order.  A lars_region holds a region's pixel count, its box
 * (row0, col0, row1, col1; half-open) and the sums of its pixels' rows and columns: the centroid is (row_sum / area,
 * col_sum / area).  Integer arithmetic throughout: the result is this definition bit for bit on every run.  R == 0 is a result.
 *
 * lars_d_region_label: mask, labels[h][w] (int32), table[capacity] and *count_dev (int64) on the device; scratch:
 * lars_region_label_scratch_bytes(h, w) bytes (0 for a raster outside the rules), 256-byte aligned.  *count_dev receives R whatever
 * the capacity is; table rows 0 .. min(R, capacity) - 1 are written (row z - 1 for region z) and nothing beyond them, so a caller
 * who reads R > capacity has labels and a table that is cut short.  capacity 0 takes table == NULL.  The labels feed
 * lars_d_zone_count / lars_d_zone_scatter as they are, with zone_bytes 4 and nzones = R (1 .. LARS_ZONES_MAX), and narrow through
 * lars_d_zone_labels_narrow.  The stages are launches on the stream; no workgroup waits for another.
 * lars_d_region_mask_f32: mask[i] = (given == NULL || given[i]) && (valid == NULL || valid[i]) && (x == NULL || x[i] > t), or
 * x[i] < t with below != 0; compared in float32 as the coverage count compares, a NaN is never inside.  x or given is required; given may be mask itself. */
typedef struct lars_region {
    int64_t area;
    int32_t bbox[4];
    uint64_t row_sum, col_sum;
} lars_region;
size_t lars_region_label_scratch_bytes(int64_t h, int64_t w);
int lars_d_region_label(const uint8_t *mask, int64_t h, int64_t w, int connectivity, int64_t min_pixels, int32_t *labels,
                        lars_region *table /* [capacity] */, int64_t capacity, int64_t *count_dev, void *scratch, void *stream);
int lars_d_region_mask_f32(const float *x /* may be NULL */, const uint8_t *given /* may be NULL */, const uint8_t *valid /* may be NULL */,
                           int64_t npix, float t, int below, uint8_t *mask, void *stream);
/* label_regions(mask): host mask in, host labels[h][w] and table[capacity] out, *n_regions = R.  label_bytes 1, 2 or 4: the width
 * of labels; 0: the narrowest of them that holds R, written to *label_bytes_out (labels then needs room for 4 bytes a pixel).
 * R above capacity, or above what label_bytes holds: LARS_ERR_INVALID with R in *n_regions (-1 after any earlier failure) and
 * nothing written to labels and table. */
int lars_h_label_regions(const uint8_t *mask, int64_t h, int64_t w, int connectivity, int64_t min_pixels, int label_bytes, void *labels,
                         int *label_bytes_out /* may be NULL */, lars_region *table /* [capacity] */, int64_t capacity, int64_t *n_regions);
/* lars_h_zonal_stats_f32 with the labels made on the device from regions instead of uploaded.  The foreground is mask (host [h][w]
 * uint8) where it is given, otherwise x > t (mode 1) or x < t (mode 2); pixels outside valid are never foreground.  The labels are
 * made, the host reads R once, and the four zone stages run with nzones = R: stats[capacity], medians[capacity][2] and
 * table[capacity] receive R rows.  capacity is 1 .. LARS_ZONES_MAX; R above it: LARS_ERR_INVALID with R in *n_regions.  R == 0
 * succeeds with nothing written.  labels_out, label_bytes and label_bytes_out as in lars_h_label_regions, labels_out may be NULL. */
int lars_h_zonal_stats_regions_f32(const float *x, const uint8_t *mask /* may be NULL */, int mode, float t, int connectivity,
                                   int64_t min_pixels, const uint8_t *valid /* may be NULL */, int64_t h, int64_t w, float threshold,
                                   int want_hist, int64_t capacity, lars_stats *stats /* [capacity] */, float *medians /* [capacity][2] */,
                                   lars_region *table /* [capacity] */, int64_t *n_regions, void *labels_out /* may be NULL */,
                                   int label_bytes, int *label_bytes_out /* may be NULL */);
/* lars_h_process_image_zones likewise: zone_stats[3][capacity], zone_medians[3][capacity][2] (row k starts at k * capacity).  Without a
 * mask the plane of index source_index (in index_mask) is compared, as the picture's white balance and mask left it. */
int lars_h_process_image_regions(const void *img, int64_t h, int64_t w, int channels, int dtype,
                                 int apply_wb, uint32_t index_mask, int want_hist,
                                 uint8_t *out_wb, float *const out_index[3],
                                 lars_stats *stats /* [3] */, float *medians /* [3][2] */,
                                 uint8_t *const out_rgba[3], const uint8_t *const cmap_lut[3],
                                 const uint8_t *valid, int use_alpha, int has_nodata, int nodata, int64_t *valid_pixels,
                                 const uint8_t *mask /* may be NULL */, int source_index, int mode, float t, int connectivity,
                                 int64_t min_pixels, int64_t capacity,
                                 lars_stats *zone_stats /* [3][capacity] */, float *zone_medians /* [3][capacity][2] */,
                                 lars_region *table /* [capacity] */, int64_t *n_regions, void *labels_out /* may be NULL */,
                                 int label_bytes, int *label_bytes_out /* may be NULL */);

/* ------------------------------------------------- region outlines (csrc/outlines.hip) */
/* The polygons of the labelled patches: the rings along the pixel borders of every region of a label raster, traced on the device.
 *
 * The definition.  labels is int32 [h][w], 0 = background, 1 .. R = regions as lars_d_region_label makes them with the same
 * connectivity: every label one connected set.  1 <= h, w and h * w < 2^29, so that an edge id fits int32.  Vertices are pixel
 * corners: corner (r, c) is the upper-left corner of pixel (r, c), 0 <= r <= h, 0 <= c <= w.  A pixel (y, x) of label L owns one
 * directed edge per side whose neighbour is not L (a neighbour outside the raster is not L), clockwise on the screen: side 0, top,
 * (y, x) -> (y, x + 1); 1, right, (y, x + 1) -> (y + 1, x + 1); 2, bottom, (y + 1, x + 1) -> (y + 1, x); 3, left, (y + 1, x) -> (y, x).
 * An edge's id is 4 * (y * w + x) + side.  The successor of an edge is the first that exists, among the edges of L that start where it
 * ends, of: the right turn (the next side of the same pixel), straight on (the same side of the next pixel along the edge), the left
 * turn (the previous side of the pixel diagonally ahead on the outer side) -- in this order with connectivity 4, in the opposite
 * order with 8: where L holds exactly two diagonal pixels of a corner, 8 crosses over and 4 stays with its own pixel.  The edges fall
 * into rings.  A ring's key is its smallest edge id; its vertices are the start corners of its edges whose predecessor has another
 * side, in ring order from the first such edge at or after the smallest edge: rows and columns alternate, no vertex lies inside a
 * straight run, a ring has an even number of vertices, 4 or more.  area2 is the exact doubled signed area, the shoelace sum over
 * (x, y) = (col, row): positive for an outer ring (clockwise on the screen), negative for a hole.  Rings are sorted by (label, key);
 * a region's first ring is its one outer ring, the others are its holes.  Integers only: the same bytes on every run.
 *
 * lars_d_region_outline_count: *edges_dev (int64, device) = E, the number of edges of the raster: what sizes the scratch.
 * lars_d_region_outline: labels, rings[ring_capacity], verts[vert_capacity][2] (row, col) and counts_dev[3] (int64: edges, rings,
 * vertices) on the device; n_labels >= the largest label (it sets the passes of the ring sort: labels above it sort by their low bits).
 * scratch: lars_region_outline_scratch_bytes(h, w, edge_capacity) bytes (0 for arguments outside the rules), 256-byte aligned: 4 bytes
 * a pixel and 35.2 bytes an edge of edge_capacity.  The counts are written whatever the capacities are; rows and vertices below the
 * capacities are written and nothing beyond them.  More edges than edge_capacity: counts_dev[0] says so, the other two counts are 0 and
 * nothing is traced.  ceil(log2(edge_capacity)) rounds of pointer doubling and some forty other launches on the stream; no workgroup
 * waits for another, and every index read from memory is range-checked before it is followed. */
typedef struct lars_outline_ring {
    int32_t label, key;            /* the region, and the ring's smallest edge id */
    int32_t start, count;          /* its vertices: verts[start .. start + count - 1] */
    int64_t area2;
} lars_outline_ring;
size_t lars_region_outline_scratch_bytes(int64_t h, int64_t w, int64_t edge_capacity);
int lars_d_region_outline_count(const int32_t *labels, int64_t h, int64_t w, int64_t *edges_dev, void *stream);
int lars_d_region_outline(const int32_t *labels, int64_t h, int64_t w, int connectivity, int64_t n_labels, int64_t edge_capacity,
                          lars_outline_ring *rings /* [ring_capacity] */, int64_t ring_capacity, int32_t *verts /* [vert_capacity][2] */,
                          int64_t vert_capacity, int64_t *counts_dev /* [3] */, void *scratch, void *stream);
/* What the host entry points below fill: the caller's arrays and their room in, the counts out (-1 until they are known).  More rings
 * or vertices than there is room for: LARS_ERR_INVALID with the counts set and nothing written to rings and verts; a caller retries
 * with that room.  No region: all three counts 0. */
typedef struct lars_outlines {
    lars_outline_ring *rings;      /* host [ring_capacity] */
    int64_t ring_capacity;
    int32_t *verts;                /* host [vert_capacity][2]: (row, col) */
    int64_t vert_capacity;
    int64_t n_rings, n_vertices, n_edges;
} lars_outlines;
/* region_outlines(mask): lars_h_label_regions, and the outlines of the labels it made, traced where they stand on the device.  The
 * host waits for R, for the edge count (which sizes a scratch area of its own) and for the ring and vertex counts. */
int lars_h_region_outlines(const uint8_t *mask, int64_t h, int64_t w, int connectivity, int64_t min_pixels, int label_bytes, void *labels,
                           int *label_bytes_out /* may be NULL */, lars_region *table /* [capacity] */, int64_t capacity, int64_t *n_regions,
                           lars_outlines *outlines);
/* lars_h_zonal_stats_regions_f32 and lars_h_process_image_regions with the outlines of the regions as well: traced after the zone
 * stages from the labels they used, which never leave the device for it.  outlines == NULL: exactly the calls above. */
int lars_h_zonal_stats_regions_outlines_f32(const float *x, const uint8_t *mask /* may be NULL */, int mode, float t, int connectivity,
                                            int64_t min_pixels, const uint8_t *valid /* may be NULL */, int64_t h, int64_t w, float threshold,
                                            int want_hist, int64_t capacity, lars_stats *stats /* [capacity] */, float *medians /* [capacity][2] */,
                                            lars_region *table /* [capacity] */, int64_t *n_regions, void *labels_out /* may be NULL */,
                                            int label_bytes, int *label_bytes_out /* may be NULL */, lars_outlines *outlines /* may be NULL */);
int lars_h_process_image_regions_outlines(const void *img, int64_t h, int64_t w, int channels, int dtype,
                                          int apply_wb, uint32_t index_mask, int want_hist,
                                          uint8_t *out_wb, float *const out_index[3],
                                          lars_stats *stats /* [3] */, float *medians /* [3][2] */,
                                          uint8_t *const out_rgba[3], const uint8_t *const cmap_lut[3],
                                          const uint8_t *valid, int use_alpha, int has_nodata, int nodata, int64_t *valid_pixels,
                                          const uint8_t *mask /* may be NULL */, int source_index, int mode, float t, int connectivity,
                                          int64_t min_pixels, int64_t capacity,
                                          lars_stats *zone_stats /* [3][capacity] */, float *zone_medians /* [3][capacity][2] */,
                                          lars_region *table /* [capacity] */, int64_t *n_regions, void *labels_out /* may be NULL */,
                                          int label_bytes, int *label_bytes_out /* may be NULL */, lars_outlines *outlines /* may be NULL */);

/* ------------------------------------------------- zone margins (csrc/zone_margin.hip) */
/* The labels of the zone stages with every zone shrunk inward by a distance: analyze_index per plot (process-images.py:492-513)
 * without the mixed pixels along a plot's edge, for callers who buffer their plots inward before they take figures.
 *
 * The definition.  labels is [h][w], zone_bytes wide (1, 2 or 4), 0 = in no zone.  For a pixel p with L(p) != 0, D2(p) is the smallest
 * (di)^2 + (dj)^2 between pixel centres to a pixel q of the raster with L(q) != L(p): background, another zone and a label above
 * nzones all differ.  Outside the raster there are no pixels: the raster's edge shrinks nothing, and a zone that fills the raster has
 * D2 = infinity.  With margin2 = m2, 0 .. LARS_ZONE_MARGIN2_MAX, the shrunk labels are L'(p) = L(p) if D2(p) > m2, else 0.  A margin
 * of m pixels is m2 = the largest n with sqrt(n) <= m in float64 (m at most 254, so that a column distance fits a byte).  The number
 * of zones does not change: a zone that vanishes is an empty zone; one that falls into pieces keeps its label.  Integers only: the
 * same bytes on every run.
 *
 * lars_d_zone_shrink: labels, g_scratch (h * w bytes) and out (a second [h][w] buffer of the same width, never labels itself) on the
 * device; two launches on the stream. */
#define LARS_ZONE_MARGIN2_MAX 64516
int lars_d_zone_shrink(const void *labels, int zone_bytes, int64_t h, int64_t w, int64_t margin2, void *g_scratch, void *out, void *stream);
/* shrink_zones(zones, margin) of a label raster: host zones[h][w] in, host out[h][w] of the same width out, nzones as in
 * lars_h_zonal_stats_f32.  Labels outside 0 .. nzones: LARS_ERR_INVALID with their number in *bad_labels (may be NULL; 0 on success,
 * -1 after any earlier failure), counted before anything is shrunk. */
int lars_h_shrink_zones(const void *zones, int zone_bytes, int64_t h, int64_t w, int64_t nzones, int64_t margin2, void *out,
                        int64_t *bad_labels /* may be NULL */);
/* lars_h_rasterize_zones with the polygons' labels shrunk on the device before they go back: shrink_zones(polygons, margin). */
int lars_h_rasterize_zones_margin(const double *verts, int64_t nverts, const int32_t *ring_starts, int64_t nrings, const int32_t *poly_starts,
                                  int64_t npolys, int64_t h, int64_t w, int zone_bytes, void *labels, int64_t margin2);
/* The calls that make zone figures, with a trailing margin2: the labels are uploaded, rasterised or labelled as in the call of the
 * same name without _margin, shrunk where they stand, and only then read by the zone stages; labels_out receives the shrunk ones, the
 * regions' table describes the regions as found.  By definition the records are those of the call without a margin on
 * lars_h_shrink_zones's raster.  Labels outside 0 .. nzones are counted and reported before anything is shrunk.  margin2 == -1: exactly
 * the call without _margin, and no kernel more. */
int lars_h_zonal_stats_margin_f32(const float *x, const void *zones, int zone_bytes, const uint8_t *valid /* may be NULL */, int64_t h, int64_t w,
                                  int64_t nzones, float threshold, int want_hist, lars_stats *stats /* [nzones] */,
                                  float *medians /* [nzones][2] */, int64_t *bad_labels, int64_t margin2);
int lars_h_zonal_stats_polygons_margin_f32(const float *x, const double *verts, int64_t nverts, const int32_t *ring_starts, int64_t nrings,
                                           const int32_t *poly_starts, int64_t npolys, const uint8_t *valid /* may be NULL */, int64_t h, int64_t w,
                                           float threshold, int want_hist, lars_stats *stats /* [npolys] */, float *medians /* [npolys][2] */,
                                           void *labels_out /* may be NULL */, int label_bytes, int64_t margin2);
int lars_h_zonal_stats_regions_margin_f32(const float *x, const uint8_t *mask /* may be NULL */, int mode, float t, int connectivity,
                                          int64_t min_pixels, const uint8_t *valid /* may be NULL */, int64_t h, int64_t w, float threshold,
                                          int want_hist, int64_t capacity, lars_stats *stats /* [capacity] */, float *medians /* [capacity][2] */,
                                          lars_region *table /* [capacity] */, int64_t *n_regions, void *labels_out /* may be NULL */,
                                          int label_bytes, int *label_bytes_out /* may be NULL */, int64_t margin2);
int lars_h_process_image_zones_margin(const void *img, int64_t h, int64_t w, int channels, int dtype,
                                      int apply_wb, uint32_t index_mask, int want_hist,
                                      uint8_t *out_wb, float *const out_index[3],
                                      lars_stats *stats /* [3] */, float *medians /* [3][2] */,
                                      uint8_t *const out_rgba[3], const uint8_t *const cmap_lut[3],
                                      const uint8_t *valid, int use_alpha, int has_nodata, int nodata, int64_t *valid_pixels,
                                      const void *zones, int zone_bytes, int64_t nzones,
                                      lars_stats *zone_stats /* [3][nzones] */, float *zone_medians /* [3][nzones][2] */,
                                      int64_t *bad_labels, int64_t margin2);
int lars_h_process_image_zones_polygons_margin(const void *img, int64_t h, int64_t w, int channels, int dtype,
                                               int apply_wb, uint32_t index_mask, int want_hist,
                                               uint8_t *out_wb, float *const out_index[3],
                                               lars_stats *stats /* [3] */, float *medians /* [3][2] */,
                                               uint8_t *const out_rgba[3], const uint8_t *const cmap_lut[3],
                                               const uint8_t *valid, int use_alpha, int has_nodata, int nodata, int64_t *valid_pixels,
                                               const double *verts, int64_t nverts, const int32_t *ring_starts, int64_t nrings,
                                               const int32_t *poly_starts, int64_t npolys,
                                               lars_stats *zone_stats /* [3][npolys] */, float *zone_medians /* [3][npolys][2] */,
                                               void *labels_out /* may be NULL */, int label_bytes, int64_t margin2);
int lars_h_process_image_regions_margin(const void *img, int64_t h, int64_t w, int channels, int dtype,
                                        int apply_wb, uint32_t index_mask, int want_hist,
                                        uint8_t *out_wb, float *const out_index[3],
                                        lars_stats *stats /* [3] */, float *medians /* [3][2] */,
                                        uint8_t *const out_rgba[3], const uint8_t *const cmap_lut[3],
                                        const uint8_t *valid, int use_alpha, int has_nodata, int nodata, int64_t *valid_pixels,
                                        const uint8_t *mask /* may be NULL */, int source_index, int mode, float t, int connectivity,
                                        int64_t min_pixels, int64_t capacity,
                                        lars_stats *zone_stats /* [3][capacity] */, float *zone_medians /* [3][capacity][2] */,
                                        lars_region *table /* [capacity] */, int64_t *n_regions, void *labels_out /* may be NULL */,
                                        int label_bytes, int *label_bytes_out /* may be NULL */, int64_t margin2);

/* ------------------------------------------------- simplified outlines (csrc/outline_simplify.hip) */
/* The rings of region outlines with fewer vertices: Douglas-Peucker with a tolerance, on the device, before the vertices cross PCIe --
 * what every vectoriser pairs with polygonising (GDAL polygonize's simplify, shapely, QGIS).
 *
 * The definition.  The input is the ring table and the vertices as lars_d_region_outline writes them: rows sorted by (label, key),
 * verts int32 (row, col).  Coordinates are 0 .. 32767 (the raster's sides are at most 32767), so every product below fits 64 bits.
 * tq is the tolerance in sixteenths of a pixel, 1 .. LARS_SIMPLIFY_TQ_MAX: floor(tolerance * 16 + 0.5) for a tolerance of 0 to 254
 * pixels; a tolerance with tq == 0 is no simplification and never reaches these entries' kernels.  For a chord from a to b and a
 * vertex p let ab = b - a, ap = p - a, len2 = |ab|^2.  If len2 == 0 then m = |ap|^2 and p is far when 256 * m > tq^2.  Otherwise let
 * dot = ap . ab; m = |ap|^2 * len2 if dot <= 0, m = |bp|^2 * len2 if dot >= len2, m = cross(ab, ap)^2 in all other cases: the squared
 * distance to the segment, not to the line, times len2; p is far when 256 * m > tq^2 * len2, which for an integer m is
 * m > (tq^2 * len2) >> 8 (m < 2^62, tq^2 * len2 < 2^56).  A ring of n vertices is the chain v[0] .. v[n] with v[n] = v[0], v[0] the
 * vertex the tracer wrote first.  Both ends are kept.  For a stretch (a, b) with b - a >= 2 take the k in (a, b) with the largest m,
 * on ties the smallest k; if that vertex is far, keep it and treat (a, k) and (k, b) the same way, otherwise the stretch is done.  The
 * first stretch has a = b in position, as stretches between the pinch points of connectivity 8 can: both take the len2 == 0 rule.
 * Collapse: a ring stays as given, with all its vertices, when its result would have fewer than 3 vertices, or when the doubled area
 * of the result is 0 or has the other sign than the ring's own shoelace sum.  The rings, their order, label and key never change;
 * start, count and area2 describe the vertices written, area2 being their shoelace sum over (x, y) = (col, row).  Nothing disappears.
 * Every vertex given lies within the tolerance of the ring written.  Integers only: the same bytes on every run.
 *
 * lars_d_outline_simplify: rings[ring_capacity], verts[vert_capacity][2] and counts_dev[3] (edges, rings, vertices: the tracer's, of
 * which the last two are read; a count above its capacity counts as 0) on the device; rings_out[ring_capacity],
 * verts_out[vert_capacity_out][2] and counts_out_dev[3] (int64: rings, vertices written, rings that stay as given) too, apart from
 * what is given.  The counts are written whatever vert_capacity_out is; vertices below it are written and nothing beyond.  h and w,
 * 1 .. 32767: coordinates are clamped to 0 .. h and 0 .. w.  A row whose start or count leaves the vertex array is a ring without
 * vertices: damaged rings give wrong rings, never an access outside the buffers.  scratch:
 * lars_outline_simplify_scratch_bytes(ring_capacity, vert_capacity) bytes (0 for arguments outside the rules: capacities 0 to 2^31 - 1),
 * 256-byte aligned: 29 bytes a vertex of vert_capacity and 58 bytes a ring of ring_capacity, and a little.  The recursion runs level
 * by level, three launches a round over all vertices; the number of rounds is the depth of the deepest ring, which is not known before
 * the run: the call WAITS for the stream once to read the longest ring's count, then enqueues eight rounds at a time and waits again
 * to read 32 bytes of status (the splits of the batch among them; 0 ends the rounds), so unlike the other
 * lars_d_ entries it returns only once the rounds are done (the last launches are still on the stream).  *rounds_out (host, may be
 * NULL): the rounds in which a stretch was split.  A ring of n vertices splits in its first n - 1 rounds at most: no round beyond the
 * longest ring's vertex count is enqueued, and a split in the last one allowed is LARS_ERR_HIP.  No workgroup waits
 * for another, and every index read from memory is range-checked before it is followed. */
#define LARS_SIMPLIFY_TQ_MAX 4064
#define LARS_SIMPLIFY_SIDE_MAX 32767
size_t lars_outline_simplify_scratch_bytes(int64_t ring_capacity, int64_t vert_capacity);
int lars_d_outline_simplify(const lars_outline_ring *rings /* [ring_capacity] */, int64_t ring_capacity, const int32_t *verts /* [vert_capacity][2] */,
                            int64_t vert_capacity, const int64_t *counts_dev /* [3] */, int64_t tq, int64_t h, int64_t w,
                            lars_outline_ring *rings_out /* [ring_capacity] */, int32_t *verts_out /* [vert_capacity_out][2] */,
                            int64_t vert_capacity_out, int64_t *counts_out_dev /* [3] */, void *scratch, int64_t *rounds_out /* may be NULL */,
                            void *stream);
/* simplify_outlines(result, tolerance): the same for host arrays, for outlines that came down earlier.  rings[n_rings] and
 * verts[n_vertices][2] in, rings_out[n_rings] and verts_out[vert_capacity_out][2] out; counts_out[3] (host) as above.  More vertices
 * than vert_capacity_out: LARS_ERR_INVALID with the counts set and nothing written; counts_out is -1 after any earlier failure. */
int lars_h_outline_simplify(const lars_outline_ring *rings, int64_t n_rings, const int32_t *verts, int64_t n_vertices, int64_t tq, int64_t h, int64_t w,
                            lars_outline_ring *rings_out, int32_t *verts_out, int64_t vert_capacity_out, int64_t *counts_out /* [3] */,
                            int64_t *rounds_out /* may be NULL */);
/* The three calls that trace outlines, with the simplification between the trace and the download: only the vertices written come
 * down.  tq 1 .. LARS_SIMPLIFY_TQ_MAX on a raster of at most 32767 a side; tq == 0: exactly the call without _simplified, and no
 * kernel more.  lars_outlines keeps its layout: n_vertices is the count written and what vert_capacity has to hold, n_edges is as
 * before, *traced_vertices (may be NULL; -1 until it is known) the count the tracer wrote.  The retry protocol when the room is short
 * stays the same, with the written count: all traced rings and vertices stay on the device, whatever the caller's room is. */
int lars_h_region_outlines_simplified(const uint8_t *mask, int64_t h, int64_t w, int connectivity, int64_t min_pixels, int label_bytes, void *labels,
                                      int *label_bytes_out /* may be NULL */, lars_region *table /* [capacity] */, int64_t capacity,
                                      int64_t *n_regions, lars_outlines *outlines, int64_t *traced_vertices /* may be NULL */, int64_t tq);
int lars_h_zonal_stats_regions_outlines_simplified_f32(const float *x, const uint8_t *mask /* may be NULL */, int mode, float t, int connectivity,
                                                       int64_t min_pixels, const uint8_t *valid /* may be NULL */, int64_t h, int64_t w,
                                                       float threshold, int want_hist, int64_t capacity, lars_stats *stats /* [capacity] */,
                                                       float *medians /* [capacity][2] */, lars_region *table /* [capacity] */,
                                                       int64_t *n_regions, void *labels_out /* may be NULL */, int label_bytes,
                                                       int *label_bytes_out /* may be NULL */, lars_outlines *outlines,
                                                       int64_t *traced_vertices /* may be NULL */, int64_t tq);
int lars_h_process_image_regions_outlines_simplified(const void *img, int64_t h, int64_t w, int channels, int dtype,
                                                     int apply_wb, uint32_t index_mask, int want_hist,
                                                     uint8_t *out_wb, float *const out_index[3],
                                                     lars_stats *stats /* [3] */, float *medians /* [3][2] */,
                                                     uint8_t *const out_rgba[3], const uint8_t *const cmap_lut[3],
                                                     const uint8_t *valid, int use_alpha, int has_nodata, int nodata, int64_t *valid_pixels,
                                                     const uint8_t *mask /* may be NULL */, int source_index, int mode, float t, int connectivity,
                                                     int64_t min_pixels, int64_t capacity,
                                                     lars_stats *zone_stats /* [3][capacity] */, float *zone_medians /* [3][capacity][2] */,
                                                     lars_region *table /* [capacity] */, int64_t *n_regions, void *labels_out /* may be NULL */,
                                                     int label_bytes, int *label_bytes_out /* may be NULL */, lars_outlines *outlines,
                                                     int64_t *traced_vertices /* may be NULL */, int64_t tq);

/* ------------------------------------------------------------------ multi-GPU */
/* One process per GPU.  RCCL (librccl.so) is loaded on first use.  unique_id is
 * LARS_COMM_ID_BYTES bytes produced by lars_comm_unique_id() on rank 0 and
 * handed to the other ranks by the launcher (file, socket, environment). */
#define LARS_COMM_ID_BYTES 128
/* LARS_OK if librccl loads with every symbol needed (a pre-flight check: a rank that cannot join must say so before the
 * others block in ncclCommInitRank) */
int lars_comm_available(void);
int lars_comm_unique_id(uint8_t *id_out);
int lars_comm_init(void **comm, int nranks, int rank, const uint8_t *unique_id);
/* number of ranks RCCL reports for the communicator (ncclCommCount): bench.py prints it as config.ranks_seen */
int lars_comm_count(void *comm, int *nranks_out);
int lars_comm_destroy(void *comm);
/* Global statistics: every rank contributes n records (device or host memory,
 * is_device says which); on return every rank holds the fold over all ranks in
 * rank order (one ncclAllGather over xGMI + a deterministic local fold). */
int lars_comm_allreduce_stats(void *comm, lars_stats *records, int64_t n, int is_device, void *stream);
/* max / sum of a double over ranks (bench timing, barriers) */
int lars_comm_allreduce_f64(void *comm, double *values_host, int64_t n, int op /*0 sum,1 max,2 min*/);
int lars_comm_barrier(void *comm);

#ifdef __cplusplus
}
#endif
#endif /* LARS_HIP_H */
