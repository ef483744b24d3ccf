/* statmc.h -- C ABI of libstatmc_hip.so: the MI355X (gfx950) implementation of StatMC's
 * per-pixel statistics accumulation and statistics-gated cross-bilateral filter.
 *
 * This is the drop-in boundary.  Every entry point names the reference interface it replaces
 * (paths relative to the StatMC repository).  Conventions:
 *   - plain C types only; device memory is passed as raw pointers (hipMalloc'ed by the caller,
 *     by statmc_malloc, or by any other HIP allocator in the same process, e.g. PyTorch-ROCm);
 *   - `stream` is a hipStream_t cast to void* (NULL = the default stream); every call is
 *     asynchronous on it, exactly like the reference enqueues on its one cv::cuda::Stream
 *     (src/statistics/estimator.h:326); statmc_synchronize() closes an iteration;
 *   - return value: 0 on success, a negative STATMC_ERR_* otherwise; statmc_last_error()
 *     returns a thread-local message.  (The reference has no error convention at these call
 *     sites -- OpenCV throws)
 *   - images are row-major with interleaved channels, exactly the cv::Mat / GpuMat layout of
 *     src/statistics/buffer.h:19-71: int32 x1 for "n", float32 x1 or x3 otherwise.  `step` is
 *     the row pitch in bytes.  The kernels walk tightly packed rows (step == cols * channels * 4), which is what
 *     the library allocates; filter<T>, pre-pass, window filter and mean-vars also take images with a longer pitch
 *     (a foreign GpuMat: they run on packed twins), the other entry points return STATMC_ERR_UNSUPPORTED for them.
 */
#ifndef STATMC_H
#define STATMC_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define STATMC_OK 0
#define STATMC_ERR_INVALID (-1)     /* bad argument (null pointer, zero size, radius too large) */
#define STATMC_ERR_UNSUPPORTED (-2) /* valid in the reference, not supported by this build */
#define STATMC_ERR_HIP (-3)         /* a HIP runtime call failed; see statmc_last_error() */
#define STATMC_ERR_NO_DEVICE (-4)   /* no gfx950 device / setup not called */

#define STATMC_MAX_BUFFERS 16  /* nBuffers per filter call (reference passes a uchar) */
#define STATMC_MAX_GBUFFERS 8

const char *statmc_last_error(void);

/* Replaces cv::cuda::stat_denoiser::setup()  (src/statistics/estimator.h:280).
 * Selects the device, uploads the Student-t quantile tables. Idempotent per device.
 *
 * All library state is kept PER DEVICE (quantile tables, significance level, filter spec, kernel
 * attributes, workspaces): a process that drives several GPUs -- one Estimator per device, the
 * one-process-eight-devices host design -- calls statmc_setup(d) once for each and every setter
 * below acts on the calling thread's current device (statmc_set_device). */
int statmc_setup(int device);

/* Compute units of the current device (0 before statmc_setup): what the launches are fitted to -- the window-sweep split,
 * and the row bands of the Upload / Denoise / Download pipeline (include/statmc_bands.hpp). */
int statmc_device_cus(void);

/* Makes `device` current for the calling thread (HIP's current device is per thread): a thread
 * other than the one that ran statmc_setup -- e.g. a render worker whose Merge*Tiles call triggers a
 * flush -- calls this before using a device other than 0.  The device must have been set up. */
int statmc_set_device(int device);

/* The reference picks the significance level at compile time by pointing `t_quantiles` at one
 * of three tables (README.md:149,158): 0 -> 0.005 (default), 1 -> 0.002, 2 -> 0.05.
 * Acts on the current device. */
int statmc_set_significance(int alpha_index);
int statmc_get_significance(void);
/* Replaces the built-in table `table` of the current device with the caller's quantiles for
 * dof = 1..n_dof (n_dof <= 4096; larger dof reuse the last entry).  table = alpha_index (0..2) for the
 * two-sided tables t_{1-alpha/2}, 3 + alpha_index for the one-sided ones t_{1-alpha} (see
 * statmc_filter_spec.sides).  The built-in tables are this build's choice; the reference's own
 * `t_quantiles` arrays live in the un-vendored stat_denoiser.cu, and a user who has them can load them
 * here; quantiles == NULL with n_dof == 0 restores the built-in table.  Call after statmc_setup()
 * (a repeated statmc_setup of the same device keeps what was loaded). */
int statmc_set_t_quantiles(int table, const float *quantiles, int n_dof);

/* Copies significance level, filter spec, window-sweep split and the quantile tables (built-in or caller-supplied) of
 * `src_device` to `dst_device`; both must have been set up.  All of these are per-device state: a host that spreads one Estimator's
 * film over several devices (statmc::FilmShards) calls this so that every block is filtered under the same rules. */
int statmc_copy_device_settings(int src_device, int dst_device);

/* ---- filter spec: everything about cv::cuda::stat_denoiser::filter<T> that the reference tree does
 * not fix (its CUDA source is in the un-vendored submodule src/ext/opencv_contrib, .gitmodules:19-21;
 * only the call sites src/statistics/estimator.cpp:437-487 and the buffer meanings README.md:317-325
 * are in the tree).  Every open choice is a field, so that pinning this build to dumps of the CUDA
 * denoiser is a search over specs (tools/fit_spec.py), not a kernel rewrite.  All-zero = this build's
 * default ("spec v2").  `sides` and `small_n` only change the pre-pass.
 * What serves which spec (statmc_last_filter_variant() names the kernel of the calling thread's last filter call;
 * times: one 1080p RGB buffer, r = 20):
 *   every gate x channel rule x border, per-pixel dof, <= 2 RGB + <= 2 one-channel G-buffers   pair-symmetric LDS kernel   1.4 - 1.9 ms
 *   ... float buffers under the asymmetric / centre gate                                       one-sided LDS kernel        2.1 ms per 3 buffers
 *   ... float buffers under the symmetric gate: two per launch (1.4 ms); an odd count >= 3     pair-symmetric + one-sided  ACRR's 5: 3.9 ms
 *       ends with its last three on the one-sided kernel ("sym_r20_f+lds_r20_f", 2.5 ms)
 *   Welch dof (dof = 1), <= 2 RGB G-buffers, any channel rule / border, RGB or float buffers   pair-symmetric Welch build  3.5 ms (1.5 per float buffer)
 *   Welch dof x one-channel G-buffers (depth, material id), RGB or float buffers               eight-plane Welch build     4.2 ms (1.85 per float buffer); block +
 *                                                                                              halo images: the 18-channel layout
 *   a clamped border on a block + halo image (multi-GPU)                                       the pair-symmetric builds + the border kernel, both on the packed image
 *   radius > 20, more than eight feature channels, G-buffers of other channel counts          general kernel ("generic")
 * All of them return the CPU oracle's results to <= 1e-5 (tests/test_gpu_parity.py::test_filter_spec_variants_match_oracle). */
#define STATMC_GATE_SYMMETRIC 0   /* member <=> fma(d, d, -(D_p + D_q)) <= 0, i.e. d^2 <= D_p + D_q        */
#define STATMC_GATE_ASYMMETRIC 1  /* member <=> fma(d, d, -D_q) <= D_p      (this build's spec v1.x)       */
#define STATMC_GATE_CENTRE 2      /* member <=> d * d <= D_p: the neighbour's mean inside the CENTRE pixel's confidence interval
                                     (Moon et al. 2013; what the reference's CUDA source computes under -DMEMFNC=1, README.md:147-150 --
                                     with significance 0.002 and the Box-Cox transform switched off, as that paragraph says) */
#define STATMC_CHANNELS_AND 0     /* every channel of an RGB buffer must pass                              */
#define STATMC_CHANNELS_JOINT 1   /* sum over channels of the left sides <= sum of the right sides        */
#define STATMC_SIDES_TWO 0        /* tabulated quantile t_{1-alpha/2, dof}                                */
#define STATMC_SIDES_ONE 1        /* t_{1-alpha, dof}                                                     */
#define STATMC_DOF_PIXEL 0        /* discriminator = t(n-1)^2 s^2/n per pixel                             */
#define STATMC_DOF_WELCH 1        /* discriminator image = s^2/n; each pair looks t up at floor(Welch-
                                     Satterthwaite dof) and tests d^2 <= t^2 (v_p + v_q)                  */
#define STATMC_BORDER_CLIP 0      /* taps outside the image are skipped                                   */
#define STATMC_BORDER_CLAMP 1     /* tap coordinates are clamped to the image (edge pixels repeat)        */
#define STATMC_SMALL_N_ACCEPT 0   /* n < 2: discriminator +inf, the pixel passes every test               */
#define STATMC_SMALL_N_EXCLUDE 1  /* n < 2: the pixel takes no part in any window                         */
typedef struct statmc_filter_spec {
    int32_t gate, channel_rule, sides, dof, border, small_n;
} statmc_filter_spec;
/* Acts on the current device; applies to every later pre-pass / window-filter call on it. */
int statmc_set_filter_spec(const statmc_filter_spec *spec);
int statmc_get_filter_spec(statmc_filter_spec *spec);
/* The spec and significance level a device has after statmc_setup: include/statmc_pinned_spec.h, which
 * tools/pin_from_dumps.sh rewrites from dumps of the CUDA build (all zero until then).  statmc_reset_filter_spec puts
 * the current device back to it; statmc_pinned_from says where it came from. */
int statmc_reset_filter_spec(void);
const char *statmc_pinned_from(void);

/* ---- window-sweep split (reproducibility across image shapes and devices).  The LDS window filters may sweep the window
 * rows of a work tile with several workgroups ("parts") whose partial sums are added afterwards; how many is chosen per
 * call from the number of tiles of the LOCAL image and the device's CU count, so that the launch fills the chip.  The
 * parts decide how a pixel's 1681 terms are grouped: two calls with a different split agree to <= 1e-6 relative L2, two
 * calls with the same split (and the same film-anchored tile grid, statmc_filter_args::film_x0 / film_y0) agree BIT FOR BIT
 * -- whatever the image shape, the region of interest, the image layout (separate images or any packed_inputs layout the
 * call's G-buffer set may travel in) or the device.  Within one image the split never depends on the
 * region a call filters (bands of the Upload / Denoise / Download pipeline = the whole-image call, bit for bit).
 * Kernel by kernel (statmc_last_filter_variant()): the pair-symmetric kernel ("sym_...") anchors its tiles and lanes in film
 * coordinates; the general kernel ("generic") sums every pixel's window in one fixed order and has no split.  The
 * ONE-SIDED LDS kernel ("lds_...": float buffers under the asymmetric / centre gate, more than two 1-channel G-buffers -- up to six
 * feature channels in all --, and the last three of an odd number >= 3 of float buffers when the sweep is in one part,
 * "sym_..._f+lds_..._f") lays its tiles from the corner of the region of interest, not on the film's grid, and ignores
 * film_x0 / film_y0.  It keeps the promise all the same, with NO alignment condition on the region's corner: a lane adds the
 * taps of a window row in ascending dx into two running sums, one for the taps with dx + (x - roi_x0) even and one for the odd
 * ones, over the window rows in ascending dy, and adds the two at the end.  Moving the corner by an odd number of columns swaps
 * the two sums and nothing else, and their sum does not care; rows, widths, the tile and the lane a pixel falls into never
 * enter.  What does enter is the KERNEL: the pair-symmetric and the one-sided kernel group a pixel's sums differently (they
 * agree to 5e-7), so the float-buffer tail makes a buffer's bits depend on the call's buffer count -- compare calls with the
 * same n_buffers -- and a forced variant (include/statmc_debug.h) is compared with itself.
 * tests/test_filter_bit_contract_gpu.py holds all of this at the C ABI, layout by layout.
 * A host that needs the blocks of a sharded film and the single-device result to be the same bits pins ONE split on every
 * device involved, the single one included:
 *     statmc_set_filter_split(statmc_filter_split_auto(film_width, film_height, radius)),
 * at the price of a launch that is no longer fitted to the block (a 1920 x 135 strip: + 34 % filter time with the whole
 * film's split of 1).  parts = 0 (default) = automatic: the fitted count, and for tile counts that leave the last round
 * of workgroups mostly empty (1280 x 720: 900 tiles on 256 CUs) more parts for the last tile rows.  Per device; acts on
 * the current device. */
int statmc_set_filter_split(int parts);
int statmc_get_filter_split(void);
/* The split the automatic choice makes on the current device for a whole image of this size (pair-symmetric kernel). */
int statmc_filter_split_auto(int width, int height, int radius);

/* Device memory + copies: the GpuMat role inside Buffer (src/statistics/buffer.h:25,57-63). */
int statmc_malloc(void **dev_ptr, size_t bytes);
int statmc_free(void *dev_ptr);   /* blocks of statmc_malloc and of statmc_malloc_placed alike */

/* ---- Device memory dealt by interference class (MI355X; no counterpart in the reference, whose buffers are plain GpuMats).
 * statmc_accumulate streams a read-once sample arena and read-modify-writes the running moments.  On MI355X every GiB of
 * device memory falls into one of three classes (most likely the three ranks behind every channel of a 12-high HBM3E stack),
 * and a stream that is READ beside WRITES into memory of its own class runs ~ 9 % slower than beside writes into another
 * class (a read-only stream does not care).  With the moments in one class and the
 * sample arenas in the others the 1080p / 256-spp launch of all stat types runs at 0.85 of the HBM peak instead of 0.76
 * (4K / 64 spp: 0.79 instead of 0.68; DESIGN.md section 4.1a, tools/experiments/acc_pool.py fastslow) -- the same kernel, the
 * same bits.  The class travels with the physical memory and HIP does not expose it, so the allocator MEASURES it: one reserved address range per device, backed GiB by GiB, every GiB probed
 * against two GiB of the allocator's own, the reference and a second target (0.2 ms each; statmc_amd/csrc/statmc_placement.hip).
 *   role STATMC_MEM_STATE   images a kernel reads AND writes per launch: n, mean, m2, m3, film-mean, film-m2 (the first 960 MiB in
 *                           the reference, the very GiB every other one is probed against, the rest in slots of its class, A)
 *   role STATMC_MEM_STREAM  read-once inputs: the sample arenas of statmc_accumulate / statmc_accumulate_tiles (all in ONE of the
 *                           other two classes while the card has room: arenas spread over both cost 2 - 3 % of the gain)
 * Blocks are 2-MiB aligned, contiguous in the address space (a block above 2 GiB is GiB slots of one class from anywhere on the
 * card, mapped side by side a second time), freed with statmc_free, and otherwise ordinary device memory.  The first call on
 * a device reserves address space and probes GiB slots until both probe levels have been seen (tens of ms); a GiB slot that
 * holds no live block is idle again (either role may take it), slots of the classes a request cannot use stay backed and idle until
 * statmc_placement_trim.  The search for a class backs at most 3 x the bytes asked for on the device so far (+ 6 GiB;
 * STATMC_PLACEMENT_MAX_GIB=<GiB> sets another budget, never above 60 % of the card) and settles for the other classes after that.
 * Blocks are valid operands of statmc_copy_rect and statmc_halo_exchange across devices: the first copy between two devices grants the
 * owner's blocks to the other device (hipMemSetAccess: hipDeviceEnablePeerAccess does not cover such memory); not IPC-shareable.  Where the probes show no contrast, the device has no virtual-memory management or memory runs short
 * the call still succeeds with memory as it comes (statmc_placement_info says so); STATMC_PLACEMENT=0 in the environment
 * makes it hipMalloc.  Not to be called while a kernel of the caller's runs (the probe competes for the memory system).
 * (ROCm 7.2 / gfx950: hipMemUnmap leaves the shaders' address translation in place -- memory mapped at an address that was mapped
 * before is not what kernels see there.  The allocator never maps an address twice: a freed window's addresses and the holes
 * statmc_placement_trim leaves are not used again, and a full range is followed by a fresh one: tools/microbench/vmm_remap.hip,
 * DESIGN.md section 4.1a.) */
#define STATMC_MEM_STATE 0
#define STATMC_MEM_STREAM 1
int statmc_malloc_placed(void **dev_ptr, size_t bytes, int role);
/* Announces how many bytes the caller is about to ask for in `role` on the current device, in however many blocks: the class search of
 * those calls is budgeted -- and, for STATMC_MEM_STREAM, the arenas' class chosen -- for all of them at once (arena by arena the first
 * 6-GiB arena settles for whichever class has six slots at hand and the later ones for what is left: arenas spread over two classes,
 * 0.77 of the HBM peak instead of 0.805).  Every statmc_malloc_placed of the role counts against it; 0 withdraws it.  Optional. */
int statmc_placement_expect(int role, size_t bytes);
typedef struct statmc_placement_info_t {
    int32_t active;          /* 1: slots are told apart and dealt by class */
    int32_t virtual_memory;  /* 1: the device maps physical allocations into reserved ranges (hipMemCreate / hipMemMap) */
    int32_t slots, probes;   /* GiB slots backed (the allocator's own included), probes run */
    int32_t slots_a, slots_b, slots_c, slots_unclear;   /* by class: A = the reference's (STATE), B = the second probe target's (STREAM), C */
    int32_t slots_idle;      /* backed, probed, dealt to no role (yet) */
    int32_t slots_as_they_came[2];   /* per role: slots dealt without the wanted class (no room for better) */
    float fast_probe_ms, slow_probe_ms;
    uint64_t slab_bytes[2], live_bytes[2];   /* per role: bytes of the slots dealt to it / bytes in live blocks */
    int32_t slots_released;  /* holes statmc_placement_trim left in the range (not counted in `slots`) */
    int32_t peer_devices;    /* devices besides the owner that the blocks are mapped for (statmc_copy_rect / statmc_halo_exchange operands) */
    int32_t peak_slots;      /* most GiB slots backed at any one time (what the class searches held before statmc_placement_trim) */
    int32_t rebased;         /* 1: the reference moved to a slot of another class, because the card's first slots were mostly of the
                                first reference's (the moments' home should be the class the card has least of) */
} statmc_placement_info_t;
int statmc_placement_info(statmc_placement_info_t *out);   /* current device */
/* Gives the memory of the idle slots of the current device (backed and probed, dealt to no role: the classes nobody asked for)
 * back to the driver; returns how many, or a negative error.  Synchronises the device.  Later statmc_malloc_placed calls back
 * and probe new slots as they need them (new slots behind the holes: released addresses are not mapped again). */
int statmc_placement_trim(void);
/* One character per GiB slot of the current device, NUL-terminated: '#' the allocator's own (the reference -- slot 0 unless
 * `rebased` -- and the second probe target), a / b / c an idle slot of that class, A / B / C one dealt to a role, S / T one dealt
 * to the state / stream role without the wanted class, '?' unclear, '_' released by statmc_placement_trim (a hole for good). */
int statmc_placement_map(char *out, int capacity);
/* Page-locked host memory for the staging side of statmc_upload / statmc_download (sample arenas
 * of the tile path, dump buffers): copies from it run at the full PCIe rate and stay asynchronous. */
int statmc_malloc_host(void **host_ptr, size_t bytes);
int statmc_free_host(void *host_ptr);
int statmc_memset(void *dev_ptr, int value, size_t bytes, void *stream);
int statmc_upload(void *dev_dst, const void *host_src, size_t bytes, void *stream);   /* Buffer::upload */
int statmc_download(void *host_dst, const void *dev_src, size_t bytes, void *stream); /* Buffer::download */
int statmc_stream_create(void **stream);
/* priority_class 0 normal, > 0 high, < 0 low.  Streams of different classes never share a hardware queue (the runtime
 * keeps one pool of GPU_MAX_HW_QUEUES queues per priority level), so the barrier packets of one cannot hold back the
 * packets of the other: what the band pipeline's copy streams need against its kernel stream (statmc_bands.hpp). */
int statmc_stream_create_with_priority(void **stream, int priority_class);
int statmc_stream_destroy(void *stream);
/* Events: order work across streams without blocking the host -- what lets Estimator::Upload / Denoise / Download
 * (src/statistics/estimator.cpp:409-489) run as a pipeline of row bands on three streams (copies in, kernels, copies
 * out) instead of one after the other.  statmc_stream_wait_event makes everything enqueued on `stream` afterwards
 * wait for the work `event` was recorded behind. */
int statmc_event_create(void **event);
int statmc_event_destroy(void *event);
int statmc_event_record(void *event, void *stream);
int statmc_stream_wait_event(void *stream, void *event);
/* Replaces cv::cuda::stat_denoiser::synchronize(stream)  (src/statistics/estimator.cpp:571-573). */
int statmc_synchronize(void *stream);

/* Device image descriptor: what one cv::cuda::PtrStepSzb entry of the reference's pointer
 * tables carries (src/statistics/estimator.cpp:35-84). */
typedef struct statmc_image {
    void *data;   /* device pointer */
    size_t step;  /* bytes per row: cols * channels * 4 (packed; what the library allocates), or more (a pitched image of the
                   * caller's: filter<T>, pre-pass, window filter and mean-vars run it through a packed twin) */
    int32_t cols; /* width  */
    int32_t rows; /* height */
} statmc_image;

/* Argument block of cv::cuda::stat_denoiser::filter<T>, in the reference's order
 * (src/statistics/estimator.cpp:437-459 for T=float, 465-487 for T=float3).  The reference
 * passes the per-buffer tables as device arrays of PtrStepSzb; here they are host arrays of
 * n_buffers descriptors (they are copied into the kernel arguments). */
typedef struct statmc_filter_args {
    uint8_t n_buffers;        /* floatBufferCounts / rgbBufferCounts [DenoiseGroup] */
    uint16_t width, height;
    float filter_ds_factor;   /* -0.5 / filtersd^2   (estimator.h:259) */
    uint8_t filter_radius;
    uint8_t denoise_film;     /* bool denoiseFilm */
    const statmc_image *n;    /* int32 x1 */
    const statmc_image *mean; /* T */
    const statmc_image *m2;   /* T */
    const statmc_image *m3;   /* T */
    const statmc_image *film; /* T: per-buffer untransformed means (tX-bY-film-mean) */
    statmc_image film_buffer; /* float3 "film" image; colour input of buffer 0 iff denoise_film */
    const statmc_image *g_buffers;     /* n_g_buffers feature-mean images */
    const uint8_t *g_channel_counts;   /* 1 or 3 per G-buffer */
    const float *g_dr_factors;         /* -0.5 / sd_g^2  (estimator.cpp:16) */
    size_t n_g_buffers;
    const statmc_image *mean_corr;     /* out, T */
    const statmc_image *discriminator; /* out, T */
    const statmc_image *film_filtered; /* out, T: tX-bY-film-mean-f */
    statmc_image film_filtered_buffer; /* out, float3 "film-f"; output of buffer 0 iff denoise_film */
    void *stream;
    /* ---- extension (all-zero = reference behaviour: filter the whole image) --------------
     * Output region of interest, used by the multi-GPU block decomposition: outputs are
     * written for x in [roi_x0, roi_x1), y in [roi_y0, roi_y1) only; the window is still
     * clipped to the full [0,width) x [0,height) local image. */
    int32_t roi_x0, roi_y0, roi_x1, roi_y1;
    /* Packed filter inputs (multi-GPU block path; data == NULL = not used).  A [height][width][15]
     * fp32 image holding, per pixel, mean_corr.rgb, discriminator.rgb, colour.rgb, g_buffers[0].rgb,
     * g_buffers[1].rgb -- the layout the halo exchange moves as one message -- or a [height][width][17]
     * image that adds two 1-channel G-buffers behind them (depth, material id: src/statistics/statpath.cpp:828-835,
     * 1096-1130; slots = the call's RGB G-buffers in argument order, then its 1-channel ones; an absent one is 0),
     * or a [height][width][16] image whose channel 15 holds the BITS of the pixel's int32 sample count: the layout for
     * STATMC_DOF_WELCH, whose pair test reads n_p and n_q (two RGB G-buffers; pair-symmetric kernel only; refused under
     * STATMC_DOF_PIXEL, as a 15- or 17-channel image is under STATMC_DOF_WELCH), or a [height][width][18] image with both:
     * channels 15, 16 the two 1-channel G-buffers, channel 17 the count's bits (STATMC_DOF_WELCH with depth / material id
     * among the G-buffers: the eight-plane Welch builds).
     * When set, statmc_window_filter (T = float3, radius <= 20, n_buffers = 1) reads its inputs from it and ignores
     * mean_corr / discriminator / film / g_buffers (g_dr_factors and, for 17 / 18 channels, g_channel_counts still describe
     * the G-buffers: 15 / 16 channels = two RGB; 17 / 18 = up to two RGB + up to two 1-channel, pair-symmetric kernel only).
     * A G-buffer set has ONE packed layout per dof rule, so that every block of a film is filtered by the build that filters the
     * whole film: exactly two RGB G-buffers and no 1-channel one travel in the 15-channel image under STATMC_DOF_PIXEL -- a
     * 17-channel image that holds just those two is refused with STATMC_ERR_UNSUPPORTED by statmc_window_filter and by the
     * pack entries below (it would run the eight-plane build, whose sums are grouped otherwise than the whole film's at r = 20
     * under the symmetric gate) -- and every other set in the 17-channel image.  Under STATMC_DOF_WELCH the two-RGB set may
     * travel in 16 or in 18 channels: both reproduce the whole film.
     * statmc_pack_filter_inputs / statmc_prepass_pack fill the owned block of such an image; the channel count is the
     * image's row pitch / (cols * 4). */
    statmc_image packed_inputs;
    /* Film coordinates of local pixel (0, 0) (multi-GPU block path; 0, 0 = the local image is the film).  The
     * window filter lays its work tiles on a grid fixed in FILM coordinates, so a pixel's sums are formed in the
     * same order whether it is filtered as part of the whole film or of a block + halo image: block-decomposed
     * results equal the single-GPU result bit for bit WHEN BOTH USE THE SAME WINDOW-SWEEP SPLIT (statmc_set_filter_split;
     * the automatic split depends on the local image's shape and the device's CU count), and to <= 1e-6 relative L2
     * under the automatic split.  (The one-sided LDS kernel does not use the film grid and needs none: the window-sweep split
     * paragraph above says why its blocks reproduce the whole film from any corner.) */
    int32_t film_x0, film_y0;
} statmc_filter_args;

/* Replace cv::cuda::stat_denoiser::filter<float> / filter<float3>: pre-pass + window filter. */
int statmc_filter_f32(const statmc_filter_args *args);
int statmc_filter_f32x3(const statmc_filter_args *args);

/* The two halves of filter<T>, separately callable (multi-GPU runs exchange halos between
 * them; the bench times them separately).  channels = 1 or 3 selects T. */
int statmc_prepass(const statmc_filter_args *args, int channels);     /* -> mean_corr, discriminator */
int statmc_window_filter(const statmc_filter_args *args, int channels); /* mean_corr, discriminator -> filtered */

/* Copies the five window-filter inputs of buffer 0 (mean_corr[0], discriminator[0], the colour
 * image -- film_buffer if denoise_film, else film[0] --, g_buffers[0], g_buffers[1]; all
 * width x height x 3) into the 15-channel image `packed` at pixel offset (dst_x0, dst_y0): the
 * owned block inside a block + halo image.  One pass, 60 B read + 60 B written per pixel.  A 17-channel `packed`
 * (row pitch cols * 68) takes up to two RGB and up to two 1-channel G-buffers (g_channel_counts says which); a
 * 16-channel one (row pitch cols * 64) also takes n[0] (channel 15: the count's bits); an 18-channel one (row pitch cols * 72)
 * takes both (the count in channel 17). */
int statmc_pack_filter_inputs(const statmc_filter_args *args, const statmc_image *packed, int dst_x0, int dst_y0);

/* statmc_prepass (T = float3, buffer 0) and statmc_pack_filter_inputs in one pass over the block:
 * reads n, mean, m2, m3, the colour image and the two G-buffers, writes the packed image; mean_corr[0] /
 * discriminator[0] are written as well when those tables are given (the reference keeps them as
 * device images), and skipped when they are NULL. */
int statmc_prepass_pack(const statmc_filter_args *args, const statmc_image *packed, int dst_x0, int dst_y0);
/* ... for n_ranges = 1 or 2 disjoint ascending row ranges {y0, y1} of the block only, in one launch (0 = the whole block). */
int statmc_prepass_pack_rows(const statmc_filter_args *args, const statmc_image *packed, int dst_x0, int dst_y0,
                             const int32_t *ranges, int n_ranges);

/* ---- film blocks on several devices of ONE process (new capability: the reference is single-GPU).
 * The Python side exchanges halos between processes with torch.distributed (RCCL send/recv); this is the same
 * exchange for a C++ host that drives all devices itself -- one Estimator per device -- with device-to-device copies
 * (peer access over xGMI, enabled on demand). */
typedef struct statmc_block {
    int32_t device;      /* HIP device that owns the block (statmc_setup must have run for it) */
    statmc_image packed; /* [block_h + halo rows][block_w + halo columns][15 | 17] fp32 on that device: the block + halo image
                            statmc_prepass_pack fills and statmc_window_filter reads; a side that lies on the film
                            border has no halo */
    void *stream;        /* the block's stream: its pack was enqueued there, the copies into it go there */
} statmc_block;
/* Fills the halo margins of every block's packed image from its neighbours.  blocks[by * gx + bx] = block (bx, by) of
 * a gx x gy grid of equal block_w x block_h blocks; radius = halo width.  Two phases, as in statmc_amd/sharding.py:
 * columns first, then rows over the widened blocks so that the corners ride along; every copy runs on the stream of
 * its destination block and is ordered behind the source block's pack / first phase by events.  Asynchronous.
 * A caller that runs exchange after exchange orders the REWRITE of a block's packed image behind its neighbours' copies
 * out of it itself (an event recorded on each neighbour's stream after this call, awaited before the next pack:
 * statmc_amd/peer.py does). */
int statmc_halo_exchange(const statmc_block *blocks, int gx, int gy, int block_w, int block_h, int radius);
/* ---- ... and between PROCESSES, one per GPU, over RCCL (north_star: "RCCL halo exchange over xGMI ... via a thin C-ABI HIP shim").
 * Every rank owns block (bx, by) = (rank % gx, rank / gx) of the gx x gy grid, packs it (statmc_prepass_pack) on block->stream and
 * calls statmc_halo_exchange_rccl with a communicator of gx * gy ranks whose rank numbers are the block numbers: point-to-point
 * sends and receives with the (at most four) neighbours, columns first, then rows over the widened block so that the corners ride
 * along -- every neighbour one hop over xGMI, no ring, no collective; a row halo is one contiguous message straight out of / into the
 * image, a column halo passes through a staging buffer.  Asynchronous on block->stream (the next statmc_window_filter on that stream
 * sees the halo); only `packed`, `device` and `stream` of *block are used.  `nccl_comm` is an ncclComm_t: the caller's own
 * (ncclCommInitRank of the RCCL the process links) or one made by statmc_rccl_comm_create.  RCCL is bound at run time (dlsym /
 * dlopen of librccl.so.1); STATMC_ERR_UNSUPPORTED where it cannot be found.  Python ranks do the same exchange through
 * torch.distributed (statmc_amd/sharding.py). */
int statmc_halo_exchange_rccl(const statmc_block *block, int gx, int gy, int block_w, int block_h, int radius, void *nccl_comm, int rank);
int statmc_rccl_available(void);                        /* 1: an RCCL library was found and bound */
int statmc_rccl_unique_id(void *id128);                 /* ncclGetUniqueId: 128 bytes, made by one rank, handed to the others by the host's own means */
int statmc_rccl_comm_create(void **nccl_comm, int n_ranks, int rank, const void *id128);   /* ncclCommInitRank on the current device (collective) */
int statmc_rccl_comm_destroy(void *nccl_comm);

/* Rectangle copy between device images of any two devices of the process (block cut / block paste of the sharded
 * path).  elem_bytes = bytes per pixel; runs on `stream`, a stream of either device (peer access is enabled in both
 * directions on first use). */
int statmc_copy_rect(const statmc_image *dst, int dst_device, int dst_x, int dst_y, const statmc_image *src,
                     int src_device, int src_x, int src_y, int width, int height, int elem_bytes, void *stream);

/* Replaces cv::cuda::stat_denoiser::calculateMeanVars<T> (commented-out call,
 * src/statistics/estimator.cpp:501-521) and its CPU stand-in (estimator.cpp:524-568):
 * film_var = film_m2 / ((n-1)*n).  row_n_quirk != 0 reproduces the CPU loop reading n once
 * per row (estimator.cpp:540,558).  n_buffers is the reference's uchar and every value of it is served, 0 (nothing to do) and
 * those above STATMC_MAX_BUFFERS included (the filter entries' limit does not apply here), with packed and with pitched images
 * alike; the buffers are computed in order, each by a launch of its own. */
int statmc_calculate_mean_vars(uint8_t n_buffers, uint16_t width, uint16_t height, int channels,
                               const statmc_image *n, const statmc_image *film_m2,
                               const statmc_image *film_var, int row_n_quirk, void *stream);

/* ---- accumulation: the GPU form of StatTile<T>::Add[Transform]SampleM{1,2,3}
 * (src/statistics/estimator.h:162-232) + Estimator::Merge[Transform]Tile
 * (src/statistics/estimator.cpp:341-407) for a whole batch of samples per pixel. ---------- */
typedef struct statmc_stat_type {
    int32_t channels;    /* 1 or 3                      (StatTypeConfig::nChannels) */
    int32_t transform;   /* Box-Cox(0.5) on the sample  (StatTypeConfig::transform) */
    int32_t max_moment;  /* 1, 2 or 3                   (StatTypeConfig::maxMoment) */
    int32_t n_samples;   /* samples per pixel in this batch */
    const float *samples; /* device, [n_samples][height][width][channels] */
    int32_t *n;          /* device state images, updated in place */
    float *mean, *m2, *m3;
    float *film_mean, *film_m2; /* transform types only; non-transform types alias mean/m2
                                   (estimator.cpp:127-137) and may pass NULL here */
    /* Optional (both or neither; max_moment 3): the accumulation's epilogue also writes the Johnson-corrected mean and the
     * discriminator of the UPDATED moments -- exactly what statmc_prepass computes from n / mean / m2 / m3 under the current device's
     * filter spec and significance level, the same bits, from the registers that hold the new moments -- so that a host whose
     * statistics live on one device goes from statmc_accumulate straight to statmc_window_filter: one launch and a 40 B/px read
     * fewer per iteration.  NULL (zero-initialised descriptors): off.  Spec or significance level changed since: call statmc_prepass. */
    float *mean_corr, *discriminator;
} statmc_stat_type;

/* The arithmetic is the reference's, operation by operation in fp32, with two stated differences:
 *   - Box-Cox takes v_sqrt_f32 (within 1 ulp of the root; the root of an exact square is exact) for pow(x, .5);
 *   - the division by the count (include/statmc_device_api.hpp, div_by_count) returns the bits of the reference's division
 *     wherever the quotient is a normal number or zero, and lies within one step of 2^-149 of it where the quotient is subnormal.
 * Samples that are not finite numbers: a negative or NaN sample leaves NaN in the Box-Cox moments like the reference; an INFINITE
 * sample leaves NaN in mean and film_mean (and in every higher moment) where the reference's division leaves inf after that
 * sample -- the quotient's residual is fma(-inf, n, inf).  Either way the element is non-finite, its pre-pass images are NaN and
 * the pixel stays out of every window. */
int statmc_accumulate(uint16_t width, uint16_t height, const statmc_stat_type *types, int n_types,
                      void *stream);

/* ---- accumulating inside the renderer's own kernel (include/statmc_device_api.hpp: statmc::device::PixelStats folds a sample
 * held in registers into a statmc_stat_type's images -- the bits of statmc_accumulate, no sample arena).  Its pre-pass store
 * needs what the accumulation's epilogue reads from the library's per-device state; a user's code object cannot see the
 * library's symbols, so the state is handed over as a value:
 *   t_table  device pointer to the current device's Student-t table of its significance level and sides (statmc_filter_spec.sides):
 *            4096 quantiles for dof = 1 .. 4096, indexed by dof - 1 (larger dof reuse the last entry)
 *   flags    the epilogue's encoding: 1 = STATMC_DOF_WELCH (the pre-pass multiplies with t = 1), 2 = STATMC_SMALL_N_EXCLUDE
 * Valid for the current device until its significance level or filter spec changes (statmc_set_significance,
 * statmc_set_filter_spec, statmc_reset_filter_spec, statmc_copy_device_settings): query again after those.  The table's
 * address stays put: statmc_set_t_quantiles rewrites it in place, so kernels enqueued after that call read the new quantiles.
 * Returns STATMC_ERR_NO_DEVICE before statmc_setup of the current device.
 * Where several lanes of a wave or several waves of a workgroup hold states of one pixel, the header's merge_lanes<G> and
 * merge_waves<NW> put them together in a fixed tree of two-part statmc_combine_statistics steps; they use nothing of the
 * library's state, so there is no C entry point for them. */
typedef struct statmc_prepass_context {
    const float *t_table;
    int32_t flags;
    int32_t reserved;   /* 0 */
} statmc_prepass_context;
int statmc_get_prepass_context(statmc_prepass_context *out);
/* The same for rows [y0, y1) of the film only (the descriptors still describe the whole film: samples
 * [n_samples][height][width][channels], whole state images).  Per-pixel work, so any split of a batch into row ranges
 * leaves the same bits; the multi-GPU step accumulates the rows next to a neighbour first and the rest while their
 * halo exchange runs. */
int statmc_accumulate_rows(uint16_t width, uint16_t height, const statmc_stat_type *types, int n_types, int y0, int y1,
                           void *stream);
/* ... and for n_ranges disjoint row ranges {y0, y1} in one launch (n_types x n_ranges <= 16). */
int statmc_accumulate_row_ranges(uint16_t width, uint16_t height, const statmc_stat_type *types, int n_types,
                                 const int32_t *ranges, int n_ranges, void *stream);

/* ---- sample arenas in the format the renderer holds them in.  sample_formats[t] says what types[t].samples points to:
 * STATMC_SAMPLES_F32, today's arenas, or STATMC_SAMPLES_F16, IEEE binary16, two bytes per element, in the same
 * [n_samples][height][width][channels] order, tightly packed.  sample_formats == NULL: every type is fp32.  ranges / n_ranges as
 * in statmc_accumulate_row_ranges; NULL / 0: the whole film (n_types x max(n_ranges, 1) <= 16).  statmc_stat_type itself does not
 * change: only the meaning of `samples` follows the type's format.
 * The call leaves, bit for bit, what statmc_accumulate (_rows, _row_ranges) leaves when given the same samples widened to fp32:
 * n, every moment, the film chain and the optional mean_corr / discriminator epilogue.  Every finite half widens to fp32 exactly,
 * subnormals included; the widening happens in registers on the way into the fold, the arena is read once and nothing is
 * allocated.  +-inf and NaN do what the fp32 path does with their widened values (not promised bit for bit).  With every format
 * fp32 the call IS the existing one: the same launch.
 * What the caller gives up is decided before the call: a value above 65504 is already inf in the caller's half, and values below
 * 6e-8 are 0 there.  Keep radiance in fp32 unless the renderer clamps it; normals, albedo, depth and material ids -- bounded,
 * low-precision quantities -- are the natural candidates for half (44 -> 28 bytes per sample of the 11-channel set, 22 all half).
 * Any 2-byte aligned half arena and any film size are accepted; arenas at 8-byte alignment (fp32 ones and the state images at
 * 16) on films whose pixel count is a multiple of 4 take the vector path, everything else goes element by element -- the same
 * bits.  STATMC_ERR_INVALID, before any launch: a format other than the two (statmc_last_error() names sample_formats), a 16-bit
 * arena at an odd address, the limits of statmc_accumulate_row_ranges.  STATMC_ERR_NO_DEVICE before statmc_setup. */
#define STATMC_SAMPLES_F32 0
#define STATMC_SAMPLES_F16 1
int statmc_accumulate_formats(uint16_t width, uint16_t height, const statmc_stat_type *types, const int32_t *sample_formats,
                              int n_types, const int32_t *ranges, int n_ranges, void *stream);

/* The same accumulation fed tile by tile, the way StatPathIntegrator::Render produces samples
 * (src/statistics/statpath.cpp:132-190: 16 x 16 tiles; 355-371: every sample of a pixel is handed to
 * the tile of every stat type; 381-388: Merge*Tiles once per tile and iteration).  Every type's
 * `samples` is an arena in which tile k owns the block starting at float offset
 * tile_offsets[k] * channels, laid out [tile_samples[k]][y1-y0][x1-x0][channels]: tile_samples[k]
 * samples for each pixel of the tile (the same count for every type; 0 = tile untouched).
 * tile_bounds = {x0,y0,x1,y1} per tile, tiles disjoint and inside the image.  All three tables are
 * device arrays.  `n_samples` of the types is ignored.  Blocks whose offset, origin and width are
 * multiples of 4 pixels (16 x 16 tiles of an image whose width is) take the vector path. */
int statmc_accumulate_tiles(uint16_t width, uint16_t height, const statmc_stat_type *types, int n_types,
                            const int32_t *tile_bounds, const int64_t *tile_offsets,
                            const int32_t *tile_samples, int n_tiles, void *stream);
/* ... with the tile arenas in the format the renderer -- or the staging of statmc::Estimator -- holds them in.  sample_formats[t]
 * is STATMC_SAMPLES_F32 or STATMC_SAMPLES_F16 and says what types[t].samples points to; NULL: every type is fp32.  Tile k's block of
 * type t starts at element offset tile_offsets[k] * channels in elements of THAT type's format -- one tile_offsets table serves
 * every type of the call, whatever their formats -- and is [tile_samples[k]][y1-y0][x1-x0][channels], tightly packed.  Everything
 * else as in statmc_accumulate_tiles.
 * The call leaves, bit for bit, what statmc_accumulate_tiles leaves for the same tables when every half arena is widened to
 * fp32: n, every moment, the film chain and the optional mean_corr / discriminator epilogue; a tile with tile_samples[k] == 0
 * keeps every bit.  Every finite half widens exactly, subnormals included; +-inf and NaN do what the fp32 path does with their
 * widened values (not promised bit for bit).  With every format fp32 the call IS statmc_accumulate_tiles: the same launch.
 * What the caller gives up is decided before the call, as for statmc_accumulate_formats; what it gains is exact: 28 instead of 44
 * bytes per pixel-sample of the 11-channel set in the arena and on the way to the device (features half), 22 all half.
 * A half type takes the vector path when its arena is 8-byte aligned, the state images 16-byte aligned and the tile's width,
 * origin, offset and the film's width multiples of 4; everything else goes element by element -- the same bits.  Half RGB rows
 * arrive by LDS-DMA, which wants more: blocks that start at 16-byte aligned addresses and hold a multiple of 8 pixels (a
 * 16-byte aligned arena, 16 x 16 tiles and their 8-wide or 8-high parts, offsets that are multiples of 8).
 * STATMC_ERR_INVALID, before any launch: a format other than the two (statmc_last_error() names sample_formats), a 16-bit arena at
 * an odd address, the limits of statmc_accumulate_tiles.  STATMC_ERR_NO_DEVICE before statmc_setup. */
int statmc_accumulate_tiles_formats(uint16_t width, uint16_t height, const statmc_stat_type *types, const int32_t *sample_formats,
                                    int n_types, const int32_t *tile_bounds, const int64_t *tile_offsets,
                                    const int32_t *tile_samples, int n_tiles, void *stream);

/* ---- arenas in which every pixel has its own sample count: what a renderer leaves that spends its samples by a per-pixel noise
 * estimate, writes the dense arena of the entries above and simply stops early on most pixels.  Everything but sample_counts means
 * what it means for statmc_accumulate_formats / statmc_accumulate_tiles_formats: arena layouts, formats (NULL = all fp32), row
 * ranges, tile tables, state pointers and the optional mean_corr / discriminator epilogue.  n_samples and tile_samples[k] become the
 * CAPACITY S of the arena or block, which keeps its dense layout.
 *   sample_counts   device image [height][width] of int32, tightly packed, indexed by film pixel in both entries.  Pixel p's
 *                   effective count is c(p) = min(max(sample_counts[p], 0), S), S = n_samples, or tile_samples[k] of the tile
 *                   that holds p.  The clamp happens before anything is derived from the count: a count outside [0, S] never
 *                   becomes an address and never reaches n.
 * Sample s of pixel p is folded iff s < c(p), in ascending s.  Arena slots with s >= c(p) may be read -- they are memory that
 * exists -- but whatever they hold (NaN, inf, uninitialised bits) reaches no state image.
 * DEFINITION, per pixel: the call leaves, bit for bit, what statmc_accumulate_tiles_formats leaves when that pixel is handed over
 * as a 1 x 1 tile with tile_samples = c(p) whose block holds the pixel's first c(p) samples in order -- equally what
 * statmc_accumulate_records leaves for those samples in that order: n (+= c(p)), every moment, the film chain and the epilogue.
 * Hence:
 *   - where every count is >= S the result is statmc_accumulate_formats' / statmc_accumulate_tiles_formats', bit for bit;
 *   - a pixel with c(p) == 0 keeps every bit of every image, mean_corr / discriminator included;
 *   - a batch may be split anywhere along s into two calls (counts min(c, k), then max(c - k, 0) on the arena advanced by k planes);
 *   - the same inputs give the same bits on every run;
 *   - the call is asynchronous on `stream`, reads nothing back and allocates nothing: no sort, no tables, no workspace.
 * sample_counts == NULL: the call IS statmc_accumulate_formats / statmc_accumulate_tiles_formats, the same launch.
 * STATMC_ERR_INVALID before any launch, statmc_last_error() naming the argument: a sample_counts address that is not 4-byte
 * aligned, and every rule the uncounted entries enforce (sample_formats, a 16-bit arena at an odd address, n_types, n_ranges, the
 * tile limits).  STATMC_ERR_NO_DEVICE before statmc_setup, after those argument checks.  Zero types, zero samples or zero tiles is
 * a no-op.
 * The vector path (a lane owns 4 consecutive pixels) needs what it needs in the uncounted entries plus a 16-byte aligned counts
 * image; everything else goes element by element, with the same bits.
 * Cost: a lane walks to the largest of its 4 counts and a wave to its longest lane, and a wave whose lanes stop at different s
 * still pulls whole memory lines of the planes it walks: the time follows the spatial coherence of the counts, not only their
 * sum.  Measured at 1920 x 1080, 11 channels, capacity 64 (profiles/accumulate_counted.jsonl): every count 64,
 * 1.09 x the time of statmc_accumulate on the same arena (1.04 against 0.95 ms: register loads where that launch streams its RGB
 * rows through LDS-DMA); one count per 16 x 16 tile, 64 on every fourth tile and 4 on the rest, 0.63 ms -- 0.32 x
 * statmc_accumulate_records on exactly the live samples (1.98 ms) and 0.66 x a launch over all 64 planes; every pixel its own
 * count, independent and uniform in 1 .. 64, 1.98 ms -- 0.61 x the records entry (3.23 ms), but 2.08 x a launch over all 64
 * planes: with incoherent counts nearly every wave walks the whole arena and most of its samples take the predicated fold.
 * The entry is ahead of the records entry on dense arenas, coherent or not; it pays off most where the counts are coherent. */
int statmc_accumulate_counted(uint16_t width, uint16_t height, const statmc_stat_type *types, const int32_t *sample_formats,
                              int n_types, const int32_t *sample_counts, const int32_t *ranges, int n_ranges, void *stream);
int statmc_accumulate_tiles_counted(uint16_t width, uint16_t height, const statmc_stat_type *types, const int32_t *sample_formats,
                                    int n_types, const int32_t *tile_bounds, const int64_t *tile_offsets,
                                    const int32_t *tile_samples, int n_tiles, const int32_t *sample_counts, void *stream);

/* ---- samples that finish anywhere: unordered (pixel, sample) records (no counterpart in the reference, whose tiles own their
 * pixels).  statmc_accumulate wants the same count for every pixel of the film, statmc_accumulate_tiles for every pixel of a
 * tile, statmc::device::PixelStats one thread that owns the pixel.  A wavefront path tracer, per-pixel adaptive sampling or a
 * sparse re-render have a queue of finished samples instead, and this entry takes that queue: 4 + 4 * channels bytes per
 * sample that exists, not per slot of a dense arena.
 *   pixels            device array of n_records entries.  Record i belongs to pixel pixels[i] = y * width + x.  Any value
 *                     outside [0, width * height) -- negative ones included -- marks a skipped record (a terminated path,
 *                     padding): it is never folded and never causes an access outside the images.
 *   types[t].samples  device, fp32, record-major [n_records][channels].  Every type shares `pixels` and n_records, as every
 *                     camera sample feeds every type in Render<T>; n_samples is ignored.  The state pointers, transform,
 *                     max_moment and the optional mean_corr / discriminator mean what they mean for statmc_accumulate.
 * The fold order is the definition: per pixel, its records are folded in ascending i, and they leave bit for bit what
 * statmc_accumulate leaves after the same samples in that order -- n, the moments, the film chain and the pre-pass epilogue.
 * So the result does not depend on how records of DIFFERENT pixels interleave, and one call over records [0, n) equals a call
 * over [0, m) followed by a call over [m, n).  A pixel without a record keeps every bit of every image, mean_corr /
 * discriminator included.  The same inputs give the same bits on every run: the records are grouped by a stable sort
 * (pixel, record index) and each pixel's run is read back in that fixed order; nothing the hardware orders -- atomic
 * arrival, wave scheduling -- reaches the fold order.
 * Limits: n_records in [0, 2^31), n_types in [0, 16]; anything else is STATMC_ERR_INVALID before any launch.  Zero records or
 * zero types is a no-op.  Counts stay below 2^24 as everywhere else; this is not checked.  Before statmc_setup:
 * STATMC_ERR_NO_DEVICE, like every compute entry.
 * Asynchronous on `stream`; nothing is read back to the host (it never learns how many pixels were touched).  The sorted
 * pairs (8 bytes per record), the per-pixel runs (8 per pixel) and the sort's temporary live in a per-(device, stream)
 * workspace that grows on demand (the only allocation on the call path, and only when a call needs more than any before it
 * on that stream) and goes with statmc_stream_destroy; like the other library workspaces it never backs or probes a placed
 * slot.
 * Cost: the grouping is linear in the records whatever their distribution.  The fold gives a pixel to one lane, and the fold of
 * one pixel is a sequential chain BY DEFINITION: the launch ends when its longest run ends, so a few pixels with tens of
 * thousands of records end it on a few lanes.  Remedy: statmc_accumulate_records_split below, which folds a long run with the
 * 64 lanes of a wave -- not the same bits as one fold, but the same statistics. */
int statmc_accumulate_records(uint16_t width, uint16_t height, const statmc_stat_type *types, int n_types,
                              const int32_t *pixels, int64_t n_records, void *stream);

/* ---- the same queue as the renderer holds it: one interleaved (array-of-structures) record per finished sample, e.g.
 * struct { int32_t pixel; float radiance[3]; float albedo[3]; float normal[3]; float depth; float id; } -- 48 bytes, or 28 with
 * the four G-buffer fields in IEEE half.  Record i starts at (char *)records + i * stride; `layout` says where in a record the
 * pixel index and every type's `channels` values lie and what they are:
 *   stride            bytes from one record to the next: a multiple of 4, at least 4
 *   pixel_offset      byte offset of the record's int32 pixel index: a multiple of 4 in [0, stride - 4]; the index means what
 *                     pixels[i] means for statmc_accumulate_records (outside [0, width * height): a skipped record)
 *   sample_offset[t]  byte offset of types[t]'s values: a multiple of the element size, the field ends at or before `stride`
 *   sample_format[t]  STATMC_SAMPLES_F32 (4-byte elements) or STATMC_SAMPLES_F16 (IEEE binary16, 2-byte elements)
 * Fields may lie in any order, leave padding between them and overlap: the same radiance field may feed a type with the
 * transform and a plain one.  types[t].samples and n_samples are ignored; `records` must be 4-byte aligned.
 * DEFINITION: the call leaves, bit for bit, what statmc_accumulate_records leaves when given pixels[i] = record i's pixel and,
 * for every type, the record-major array of that type's field with half fields widened to fp32 (every finite half widens
 * exactly, subnormals included).  Everything that entry promises carries over: the per-pixel fold in ascending i, skipped
 * records that never become an address, untouched pixels that keep every bit, a call over [0, n) equal to calls over [0, m)
 * and [m, n), the same bits on every run, the optional pre-pass epilogue, asynchronous on `stream`, nothing read back, the
 * same per-(device, stream) workspace.  The records are read in place: nothing is de-interleaved or copied first.
 * STATMC_ERR_INVALID before any launch (statmc_last_error() names the argument): the n_records and n_types limits of
 * statmc_accumulate_records; layout == NULL with n_types > 0 or n_records > 0; a stride, records address, pixel_offset,
 * sample_offset or sample_format outside the rules above.  Zero records or zero types is a no-op; STATMC_ERR_NO_DEVICE before
 * statmc_setup.
 * Why a second entry: a shuffled record of the per-array entry costs one memory line per stat type, an interleaved one costs
 * one or two in all. */
typedef struct statmc_record_layout {
    int32_t stride;             /* bytes from one record to the next */
    int32_t pixel_offset;       /* byte offset of the record's int32 pixel index */
    int32_t sample_offset[16];  /* per types[t]: byte offset of its `channels` values */
    int32_t sample_format[16];  /* per types[t]: STATMC_SAMPLES_F32 or STATMC_SAMPLES_F16 */
} statmc_record_layout;

int statmc_accumulate_records_interleaved(uint16_t width, uint16_t height,
        const statmc_stat_type *types, int n_types,
        const void *records, const statmc_record_layout *layout,
        int64_t n_records, void *stream);

/* ---- the same two queues with heavy-tailed counts: a pixel's LONG run is split over the 64 lanes of a wave.  The argument lists
 * are statmc_accumulate_records' and statmc_accumulate_records_interleaved's plus split_above in front of `stream`.
 * DEFINITION, per pixel.  Pixel p's run is its live records of this call in ascending record index, exactly as for
 * statmc_accumulate_records; c is its length.
 *   c <= split_above  the pixel is folded as statmc_accumulate_records folds it: the same bits.  c == 0: untouched, every bit of
 *                     every image stays, mean_corr / discriminator included.
 *   c >  split_above  the run is cut into STATMC_RECORDS_SPLIT_LANES = 64 contiguous chunks of L = ceil(c / 64) records: slot j
 *                     owns the run's positions [min(j L, c), min((j + 1) L, c)); trailing slots may be empty.  Slot 0 starts
 *                     from the pixel's stored state, every slot j > 0 from the state of no samples (n = 0, all moments 0), and
 *                     each folds its chunk in order.  The 64 states are merged in the tree of statmc::device::merge_lanes<64>
 *                     (include/statmc_device_api.hpp):
 *                         for stride = 1, 2, 4, 8, 16, 32: for every j with j % (2 stride) == 0: slot[j].merge(slot[j + stride])
 *                     and slot 0's result is stored -- with mean_corr / discriminator given, the pre-pass of the merged moments
 *                     too.
 * Through the other entries, a split pixel holds bit for bit what these calls leave: statmc_accumulate_records of chunk 0 into
 * the stored state; statmc_accumulate_records of chunk j into zeroed images, j = 1 .. 63; 63 two-part
 * statmc_combine_statistics calls in the tree's order (dst = set j, src = set j + stride); statmc_prepass of the result where
 * the epilogue is asked for.  The chunks and the tree are functions of c alone: which lanes, waves or compute units did the work
 * reaches no bit.  The interleaved entry leaves, bit for bit, what the per-array split entry leaves on the de-interleaved arrays
 * with half fields widened -- the relation of the two entries above.
 * Carried over from those entries: dead records (any pixel value outside [0, width * height)) are never folded and never become
 * an address; the result does not depend on how records of DIFFERENT pixels interleave; the same inputs and the same
 * split_above give the same bits on every run; asynchronous on `stream`, nothing read back, the same per-(device, stream)
 * workspace, which may grow; zero records or zero types is a no-op; the n_records / n_types / layout limits and their
 * STATMC_ERR_INVALID messages; STATMC_ERR_NO_DEVICE before statmc_setup, after the argument limits.
 * NOT carried over: for a split pixel a call over [0, n) is NOT a call over [0, m) followed by one over [m, n) (the chunks are
 * those of the call's run), and the bits differ from statmc_accumulate_records' in the last places: the statistics are the
 * same, the fold order is not.
 * split_above < 1 is STATMC_ERR_INVALID before any launch (statmc_last_error() names split_above).  With split_above at least
 * the longest run (INT32_MAX: never split) every bit is statmc_accumulate_records'.  STATMC_RECORDS_SPLIT_DEFAULT is the
 * measured choice.
 * A single pixel beyond what 64 lanes handle well (millions of records) stays the caller's business: deal its records to
 * several states (several calls into several sets of images) and put them together with statmc_combine_many. */
#define STATMC_RECORDS_SPLIT_LANES 64
#define STATMC_RECORDS_SPLIT_DEFAULT 256
int statmc_accumulate_records_split(uint16_t width, uint16_t height, const statmc_stat_type *types, int n_types,
                                    const int32_t *pixels, int64_t n_records, int32_t split_above, void *stream);
int statmc_accumulate_records_interleaved_split(uint16_t width, uint16_t height, const statmc_stat_type *types, int n_types,
                                    const void *records, const statmc_record_layout *layout, int64_t n_records,
                                    int32_t split_above, void *stream);

/* ---- combining independently accumulated statistics (no counterpart in the reference, whose renders can only be split by
 * --baseseed and then not put back together: src/main/pbrt.cpp:71,165-168).  Per pixel and channel, part A in `dst`, part B
 * in `src`, n = nA + nB, delta = meanB - meanA (Chan et al. 1979, Pebay 2008):
 *     mean = meanA + delta nB / n
 *     m2   = m2A + m2B + delta^2 nA nB / n
 *     m3   = m3A + m3B + delta^3 nA nB (nA - nB) / n^2 + 3 delta (nA m2B - nB m2A) / n
 * film_mean / film_m2 follow the mean / m2 lines with their own delta and the same counts.  These are the reference's Meng
 * update (src/statistics/estimator.h:162-205, "m3 uses the updated m2") when B is one sample: with nB = 1, m2B = m3B = 0,
 * d = delta and dN = d / n,
 *     m2:  d^2 nA / n                          = d (d - dN)                                       (d - dN = d nA / n)
 *     m3:  d^3 nA (nA - 1) / n^2 - 3 dN m2A    = -3 dN (m2A + d^2 nA / n) + d (d^2 - dN^2)
 *          since n^2 - 1 - 3 nA = nA (nA - 1) for n = nA + 1, and m2A + d^2 nA / n is the updated m2.
 * fp32 operation order (ints nA, nB; fA = (float)nA, fB = (float)nB, nf = (float)(nA + nB); r = refined 1 / nf and
 * div(x) = x / nf rounded as the accumulation divides by its count; every operation rounds once, nothing is contracted):
 *     d = meanB - meanA;  t = div(d * fB);  q = d * fA;  u = div(d)
 *     mean = meanA + t
 *     m2   = (m2A + m2B) + q * t
 *     m3   = ((m3A + m3B) + (q * t) * ((fA - fB) * u)) + (3 * u) * (fA * m2B - fB * m2A)      (m2A, m2B: before the call)
 * Exact cases, per pixel: nB == 0 leaves dst's bits unchanged; otherwise nA == 0 makes dst a bit copy of src; n is the
 * integer sum; constant samples (delta = 0, m2 = m3 = 0 on both sides) give m2 = m3 = 0 exactly.
 * Counts must sum below 2^24, the range in which (float)n and the refined reciprocal are exact; this is not checked per pixel.
 *
 * Each entry reuses statmc_stat_type for both sides:
 *   - max_moment picks the fields: 1 = mean, 2 = mean and m2, 3 = mean, m2 and m3; dst and src agree on channels and max_moment;
 *   - film_mean / film_m2 are combined when non-NULL and not the same pointers as mean / m2 (a non-transform type whose film
 *     images alias its moments, estimator.cpp:127-137, is combined once); film_m2 without a film_mean of its own is an error;
 *   - dst.samples, dst.n_samples and both `transform` fields are ignored, as are src.mean_corr / src.discriminator;
 *   - dst.mean_corr / dst.discriminator (both or neither; max_moment 3 and own counts): the call's epilogue writes the
 *     pre-pass of the combined moments there under the device's current spec and significance level -- the bits
 *     statmc_prepass computes from them, like the accumulation's epilogue;
 *   - count_of = -1: dst.n / src.n are the entry's counts, and dst.n becomes nA + nB.  count_of = k >= 0: the entry is
 *     weighed with entry k's counts AS THEY WERE BEFORE THE CALL, whatever the entry order; dst.n and src.n are NULL and
 *     entry k has count_of = -1.  This is how the "film" RGB image is combined (an M1 mean weighted by t0-b0-n: with StatMC's
 *     box filter Film's weight sum per pixel is that count, film.h:152-190, statpath.cpp:355-358, apart from samples that
 *     land exactly on a pixel edge), and G-buffer means of a dump that carries no n of their own (every camera sample feeds
 *     radiance b0 and every G-buffer, statpath.cpp:357-371).
 * No dst image may be its src counterpart; no two entries may own the same count image.  Images are packed width x height
 * planes like statmc_accumulate's.  n_entries = 0 is a no-op, at most 16 (statmc::kMaxStatTypes); one launch serves all.
 * Asynchronous on `stream`; both states on the current device (copy first with statmc_copy_rect). */
typedef struct statmc_combine_entry {
    statmc_stat_type dst; /* updated in place; samples / n_samples / transform ignored */
    statmc_stat_type src; /* read only; mean_corr / discriminator ignored */
    int32_t count_of;     /* -1: dst.n / src.n are this entry's counts, and dst.n is updated.
                             k >= 0: weigh with entry k's counts as they were before the call;
                             dst.n and src.n must be NULL; entry k must have count_of == -1 */
} statmc_combine_entry;

int statmc_combine_statistics(uint16_t width, uint16_t height, const statmc_combine_entry *entries, int n_entries,
                              void *stream);

/* ---- the same for K parts: dst (part 0) and n_sources further parts, one pass over memory.  The call leaves in every dst
 * exactly the bits that this sequence leaves:
 *     for k = 0 .. n_sources - 1: one statmc_combine_statistics call whose entries are (dst, srcs[k], count_of)
 * -- a left fold in array order, per pixel and channel -- where that sequence moves 3 (K - 1) B bytes for K = n_sources + 1
 * parts of B bytes per pixel and this call (K + 1) B: every part read once, dst written once.  Everything said above holds
 * per source, so:
 *   - per source, nB == 0 keeps the running bits and nA == 0 takes the source's bits; n becomes the integer sum;
 *   - source k of an entry that borrows counts is weighed with its owner's running count, dst.n plus the counts of sources
 *     0 .. k - 1, and with the owner's srcs[k].n: source k of every entry belongs to the same part k.  The owner's dst.n is
 *     written once, at the end;
 *   - film planes that alias the moments are combined once; the dst.mean_corr / dst.discriminator epilogue runs once, on the
 *     final moments;
 *   - every srcs[k] agrees with dst on channels and max_moment; no dst image may be an image of one of its sources; no two
 *     entries may own the same count image (STATMC_ERR_INVALID, before anything is launched).
 * n_sources = 0 or n_entries = 0 is a no-op; n_sources <= STATMC_MAX_COMBINE_SOURCES, n_entries <= 16, every pair works.
 * `srcs` is a host array that the call has read when it returns.  The source tables travel as kernel arguments, so a call
 * whose tables do not fit one launch (more than 90 / n_sources chains, a chain being an entry's moments or its film images
 * of their own) becomes several launches on `stream`, the chains that only read counts first.  Asynchronous on `stream`;
 * all states on the current device. */
#define STATMC_MAX_COMBINE_SOURCES 15
typedef struct statmc_combine_many_entry {
    statmc_stat_type dst;         /* part 0, updated in place; as statmc_combine_entry::dst */
    const statmc_stat_type *srcs; /* host array of n_sources read-only parts, in fold order */
    int32_t count_of;             /* as in statmc_combine_entry */
} statmc_combine_many_entry;

int statmc_combine_many(uint16_t width, uint16_t height, const statmc_combine_many_entry *entries, int n_entries,
                        int n_sources, void *stream);

/* ---- pooling k x k blocks of pixels into a coarser film (no counterpart in the reference): the statistics of the samples of
 * NEIGHBOURING pixels put together, where the two calls above put together samples of the same pixel.  k is 2, 4 or 8.  The fine
 * film (src) has width x height pixels, the coarse one (dst) Wc x Hc with Wc = ceil(width / k), Hc = ceil(height / k); both are
 * packed planes like every image of this header.
 * DEFINITION.  Coarse pixel (X, Y) has k * k slots.  Slot j holds the state of fine pixel (k X + dx, k Y + dy) with
 * j = Morton(dx, dy): bit i of dx is bit 2 i of j, bit i of dy is bit 2 i + 1 (k = 2: slots 0 .. 3 are (0,0) (1,0) (0,1) (1,1)).
 * A slot whose fine pixel lies outside the film holds the state of no samples (n = 0, every field 0).  The coarse state is the
 * balanced tree of statmc::device::merge_lanes (include/statmc_device_api.hpp) over those slots:
 *     for stride = 1, 2, 4, ... < k * k:
 *         for every slot j with j % (2 stride) == 0:   slot[j].merge(slot[j + stride])        (A = slot j, B = slot j + stride)
 * with slot 0's result stored.  Through the other entries: the result is, bit for bit, what k * k part states of size Wc x Hc --
 * part j holding slot j of every coarse pixel -- give when combined by two-part statmc_combine_statistics calls in exactly that
 * order (dst = part j, src = part j + stride).  Every rule of that call holds per merge: nB == 0 keeps A's bits, otherwise
 * nA == 0 takes B's, n is the integer sum; counts must sum below 2^24 per block, which is not checked.  Hence:
 *   - dst.n is the sum of the block's counts;
 *   - a block with one live pixel is a bit copy of that pixel's state, wherever in the block it lies;
 *   - a block without a live sample keeps the bits of its slot 0, fine pixel (k X, k Y), which always lies inside the film;
 *   - the slots are in Morton order, so the tree's levels alternate pairs along x and pairs along y, and pooling by 2 and
 *     pooling the result by 2 again IS the tree of pooling by 4: pool_a(pool_b(film)) == pool_ab(film) bit for bit for
 *     a b <= 8, partial blocks at the right and bottom edge included.  A pyramid holds the same bits whichever way it was built
 *     (a row-major slot order would not give this);
 *   - it is NOT the left fold in slot order that statmc_combine_many computes from the same parts: fp32 addition is not
 *     associative, and the two orders differ in the last bits.
 * Each entry reuses statmc_stat_type for both sides as statmc_combine_entry does: channels and max_moment pick the planes and
 * must agree; film_mean / film_m2 are pooled when non-NULL and not the same pointers as mean / m2, and dst and src agree on which
 * of them they have; samples, n_samples and transform are ignored, as are src.mean_corr / src.discriminator.  dst is WRITTEN:
 * what it held is not read.  count_of = -1: the entry owns src.n and dst.n.  count_of = q >= 0: every merge of the entry is
 * weighed with entry q's counts of the same two sub-trees (the slots' counts are read from entry q's src.n); dst.n and src.n are
 * NULL and entry q has count_of = -1 -- the "film" RGB image and the G-buffer means of a dump without counts, as for
 * statmc_combine_statistics.  dst.mean_corr / dst.discriminator (both or neither; max_moment 3 and own counts): the epilogue
 * writes the pre-pass of the pooled moments under the device's current spec and significance level, the bits statmc_prepass
 * computes from the pooled images.
 * One launch serves all entries; n_entries <= 16, n_entries = 0 is a no-op.  Asynchronous on `stream`, nothing is allocated or
 * read back; both films on the current device.
 * STATMC_ERR_INVALID before any launch, statmc_last_error() naming the argument: k not 2, 4 or 8; a zero width or height;
 * n_entries outside [0, 16] or NULL entries with n_entries > 0; channels not 1 or 3, max_moment not 1..3; dst and src
 * disagreeing on channels, max_moment or their film planes; a NULL plane the entry needs; film_m2 without a film_mean of its own;
 * a broken count_of rule; one of mean_corr / discriminator alone, or either with max_moment < 3 or borrowed counts; the byte range
 * of any dst plane (coarse size) overlapping that of any src plane (fine size) of any entry; two entries writing the same dst
 * plane or owning the same dst count image.  STATMC_ERR_NO_DEVICE before statmc_setup, after those checks.
 * Measured at 1920 x 1080 on the 11-channel set plus "film": DESIGN.md 4.2b, profiles/pool_statistics.jsonl. */
typedef struct statmc_pool_entry {
    statmc_stat_type dst; /* coarse film, ceil(width/k) x ceil(height/k), WRITTEN: what it held is not read */
    statmc_stat_type src; /* fine film, width x height, read only */
    int32_t count_of;     /* as in statmc_combine_entry */
} statmc_pool_entry;

int statmc_pool_statistics(uint16_t width, uint16_t height, int k, const statmc_pool_entry *entries, int n_entries, void *stream);

/* ---- the way back up (no counterpart in the reference): the FILTERED image of a film pooled k x k, brought onto the fine film by a
 * statistics-gated joint upsampling.  `fine` and `coarse` are the argument blocks the filter entries take for the two films; the
 * coarse one has been through statmc_prepass and statmc_window_filter, the fine one through statmc_prepass (or a fused epilogue).
 * One HBM-bound launch per buffer on fine->stream; the fine film is only read, nothing is allocated or read back.
 *   read from `fine`, per buffer b < n_buffers: mean_corr[b], discriminator[b], the colour image (film_buffer if denoise_film and
 *     b == 0 and channels == 3, else film[b]), g_buffers / g_channel_counts / g_dr_factors / n_g_buffers, the ROI (all-zero: the
 *     whole film), stream;
 *   read from `coarse`: mean_corr[b], discriminator[b], g_buffers, and its filtered image (film_filtered_buffer if denoise_film and
 *     b == 0 and channels == 3, else film_filtered[b]);
 *   written: the fine filtered image of every buffer, for the pixels of the ROI.  Nothing else.
 * The filter spec is the current device's (gate, channel_rule, border; sides and small_n are already inside the images).
 * DEFINITION, per fine pixel p = (x, y) and buffer; every float operation rounds once, in this order, no contraction:
 *   t = 2 x + 1 - k;  X0 = floor(t / 2k) (-1 in the left half-block);  a = t - 2k X0, odd, in [1, 2k - 1];
 *   wx[0] = (2k - a) / 2k, wx[1] = a / 2k (dyadic: exact);  the same in y.  The tents sit on the regular grid of block centres; a
 *   partial edge block does not move its centre.
 *   Candidates Q = (X0 + i, Y0 + j) in the order (j, i) = (0,0) (0,1) (1,0) (1,1).  Outside the coarse image: skipped under
 *   STATMC_BORDER_CLIP, coordinates clamped under STATMC_BORDER_CLAMP.  A candidate that is not a valid pixel -- corrected mean and
 *   FILTERED colour finite, discriminator not NaN, every G-buffer value finite -- is skipped.
 *   (p, Q) is a member by the window filter's pair test under STATMC_DOF_PIXEL: p supplies D_p, Q supplies D_q, with the fma where
 *   the gates above have it, all three gates and both channel rules.
 *   e = 0;  per G-buffer: dist2 = d0 d0, then fma(dc, dc, dist2) per further channel;  e = fma(dr_g, dist2, e), G(p) fine, G(Q) coarse;
 *   w = (wx[i] wy[j]) exp(e);   sum_w += w;   acc[c] += w * filtered(Q)[c]   (multiply and add rounded separately).
 *   out[c] = acc[c] / sum_w if sum_w > 0, else the bits of p's own colour; a p that is not a valid pixel (its own colour in the
 *   colour's place) passes its colour through bit for bit, NaN included.
 * exp may be the hardware exponential (<= 1e-5 relative L2 against a double evaluation, as every filter kernel here); it is exactly 1
 * where e == 0 -- no G-buffers, all factors 0, equal features --, and there the whole result is this definition bit for bit.
 * STATMC_ERR_INVALID, statmc_last_error() naming the argument: a NULL block; k not 2, 4 or 8; channels not 1 or 3; a coarse size
 * other than ceil(width / k) x ceil(height / k); n_buffers, n_g_buffers or a channel count differing between the blocks; a NULL table
 * or image; a bad ROI; an output overlapping any image the call reads.  STATMC_ERR_UNSUPPORTED, nothing written: STATMC_DOF_WELCH
 * (its discriminator image is not a discriminator); packed_inputs on either side; pitched images; more than two RGB or two
 * one-channel G-buffers.  STATMC_ERR_NO_DEVICE before statmc_setup, after those checks.  One level per call: a host may chain
 * 8 -> 4 -> 2 -> 1, each call defined on its own.  Measured: DESIGN.md 4.2h, profiles/upsample.jsonl. */
int statmc_upsample_filtered(const statmc_filter_args *fine, const statmc_filter_args *coarse, int k, int channels);

/* ---- planning per-pixel sample counts from the statistics (no counterpart in the reference): what feeds the sample_counts of
 * statmc_accumulate_counted / statmc_accumulate_tiles_counted.  Two entries: a pointwise noise score, and the allocation of a
 * budget by a score image.  Minimising the summed variance of the mean, sum_p s_p^2 / (n_p + c_p), under a fixed sum of c_p gives
 * n_p + c_p proportional to s_p, clamped per pixel: one scalar level, found by water-filling.  All images are packed
 * width x height planes like every image of this header.
 *
 * statmc_sample_scores: statistics -> score image.  channels is 1 or 3; film_mean / film_m2 are the raw-sample Welford planes of a
 * stat type (for a non-transform type its mean / m2).
 * DEFINITION, per pixel; every operation is one fp32 rounding in this order, nothing is contracted, `/` and sqrt are the correctly
 * rounded IEEE quotient and root:
 *     n < 2:      score = +inf                    (a pixel nobody can judge yet takes the maximum)
 *     otherwise   fn = (float)(n - 1);  v = film_m2[0] / fn  (+ film_m2[1] / fn) (+ film_m2[2] / fn), added in channel order;
 *                 sd = sqrt(v)
 *       STATMC_SCORE_ABSOLUTE   score = sd
 *       STATMC_SCORE_RELATIVE   score = sd / (eps + a),  a = |film_mean[0]| (+ |film_mean[1]|) (+ |film_mean[2]|) in channel order
 * Non-finite or negative statistics pass through as the arithmetic has it (NaN stays NaN, sqrt of a negative sum is NaN);
 * statmc_plan_samples says what such a score means.  So a numpy float32 restatement gives the same bits.  Planes that are all
 * 16-byte aligned move four pixels per lane; any other alignment, and the film's last partial group of four, go pixel by pixel to
 * the same bits.
 * STATMC_ERR_INVALID before any launch, statmc_last_error() naming the argument: a zero width or height; channels not 1 or 3; a
 * metric other than the two; with STATMC_SCORE_RELATIVE an eps that is not positive and finite (eps is ignored otherwise); a NULL or
 * not 4-byte aligned image; score overlapping n, film_mean or film_m2.  STATMC_ERR_NO_DEVICE before statmc_setup, after those checks.
 * Asynchronous on `stream`. */
#define STATMC_SCORE_ABSOLUTE 0
#define STATMC_SCORE_RELATIVE 1
int statmc_sample_scores(uint16_t width, uint16_t height, int channels, int metric, float eps,
                         const int32_t *n, const float *film_mean, const float *film_m2,
                         float *score, void *stream);

/* statmc_plan_samples: score image + counts so far + budget -> count image.  `score` is statmc_sample_scores' or the renderer's own
 * metric; n is the per-pixel count so far, NULL meaning 0 everywhere; 0 <= c_min <= c_max <= 2^20 and budget >= 0.
 * DEFINITION.  A pixel's class by its score s:  saturated  s > 2^60 (+inf included);  live  2^-60 <= s <= 2^60;  dead  everything
 * else (0, negative, tiny, NaN).  A level is the float of bit pattern u in [U_LO, U_HI] = [0x20000000, 0x5F000000], 2^-63 .. 2^63, so
 * every product below is a normal number and denormal modes reach no bit.  Per pixel p:
 *     live:       t = fl32(float_from_bits(u) * s);   N = (t >= 2^30) ? 2^30 : (int)ceil(t);
 *                 c_p(u) = clamp(N - clamp(n_p, 0, 2^30), c_min, c_max)
 *     saturated:  c_p(u) = c_max            dead:  c_p(u) = c_min
 * T(u) = sum_p c_p(u) is an exact integer, non-decreasing in u (rounded multiplication, ceil and clamp are monotone).
 *     budget <= T(U_LO):   sample_counts = c(U_LO), status 1, level_bits = U_LO   (the floor already spends the budget or more)
 *     budget >  T(U_HI):   sample_counts = c(U_HI), status 2, level_bits = U_HI   (the ceiling cannot spend it)
 *     otherwise:           u* = the smallest u with T(u) >= budget, level_bits = u*, status 0, and the overshoot of that last float
 *                          step is trimmed in raster order:  base_p = c_p(u* - 1),  d_p = c_p(u*) - base_p,  R = budget - T(u* - 1),
 *                          E_p = the sum of d_q over the pixels q < p in row-major order,
 *                          sample_counts[p] = base_p + clamp(R - E_p, 0, d_p)
 * result->total is the sum of sample_counts, n_live / n_saturated the number of pixels of those classes.  Hence:
 *   - with status 0, total == budget to the sample: a renderer sizes its arena or its record queue by it;
 *   - every count lies in [c_min, c_max];
 *   - the same inputs give the same bits on every run: every reduction is an integer sum, so no order reaches a bit;
 *   - on a film of one constant live score all pixels step together, and the trim hands the last samples to the first pixels in
 *     raster order;
 *   - the image is what statmc_accumulate_counted / statmc_accumulate_tiles_counted take as sample_counts.
 * Asynchronous on `stream`; nothing is read back and nothing allocated.  The caller owns `workspace`, at least
 * statmc_plan_samples_workspace(width, height) bytes (a pure function, no device needed) and 8-byte aligned; the call zeroes it on
 * `stream` and leaves nothing of use in it.  `result` is device memory, 8-byte aligned, written by the call.  The search runs on the
 * device: five passes that evaluate T at 64 levels each, every workgroup deriving its levels from the totals of the pass before,
 * then a three-launch prefix sum; no kernel waits for another workgroup.
 * STATMC_ERR_INVALID before any launch, statmc_last_error() naming the argument: a zero width or height; NULL score, sample_counts,
 * result or workspace; score, n or sample_counts not 4-byte aligned, result or workspace not 8-byte aligned; c_min / c_max outside
 * 0 <= c_min <= c_max <= 2^20; a negative budget; workspace_bytes below the helper's answer; sample_counts overlapping score, n,
 * result or the workspace, or result overlapping the workspace.  STATMC_ERR_NO_DEVICE before statmc_setup, after those checks.
 * Measured at 1920 x 1080 and 3840 x 2160: DESIGN.md 4.2c, profiles/plan_samples.jsonl. */
typedef struct statmc_plan_result { /* device, written by the call */
    int64_t total;       /* sum of sample_counts */
    int64_t budget;      /* as asked */
    uint32_t level_bits; /* the level u* (U_LO with status 1, U_HI with status 2) */
    int32_t status;      /* 0 exact; 1 budget below the floor; 2 budget above the ceiling */
    int32_t n_live, n_saturated;
} statmc_plan_result;

size_t statmc_plan_samples_workspace(uint16_t width, uint16_t height); /* bytes; pure, no device needed */
int statmc_plan_samples(uint16_t width, uint16_t height, const float *score, const int32_t *n,
                        int64_t budget, int32_t c_min, int32_t c_max,
                        int32_t *sample_counts, statmc_plan_result *result,
                        void *workspace, size_t workspace_bytes, void *stream);

/* ---- the error of the mean as a score image, and the counts that bring it to a tolerance (no counterpart in the reference).
 * statmc_sample_scores' sample standard deviation converges to the pixel's true sigma: it is what the budget plan spends by, and it
 * does not fall as samples arrive.  A stopping rule needs a quantity that does: the standard error of the mean, sqrt(v / n), or the
 * half-width of the mean's confidence interval, that times the Student-t quantile at n - 1 degrees of freedom.
 *
 * statmc_error_scores: channels, metric, eps and the images are statmc_sample_scores'.  `table` is STATMC_ERROR_NO_TABLE (the standard
 * error) or 0..5, numbered as in statmc_set_t_quantiles, alpha_index + 3 * sides: the score is the half-width of that confidence
 * interval.  T[table] is the CURRENT DEVICE's table as it stands when the call is made, quantiles loaded by the caller included.
 * DEFINITION, per pixel; every operation is one fp32 rounding in this order, nothing is contracted, `/` and sqrt are the correctly
 * rounded IEEE quotient and root:
 *     n < 2:      score = +inf
 *     otherwise   fn1 = (float)(n - 1);  v = film_m2[0] / fn1  (+ film_m2[1] / fn1) (+ film_m2[2] / fn1)    (statmc_sample_scores' v)
 *                 vm = v / (float)n;  e = sqrt(vm)
 *       table >= 0:               q = T[table][min(n - 1, 4096) - 1];  e = q * e
 *       STATMC_SCORE_RELATIVE:    e = e / (eps + a),  a as in statmc_sample_scores
 *                 score = e
 * Non-finite or negative statistics pass through as the arithmetic has it.  The library is built without a denormal flush:
 * subnormal m2, quotients and products are part of the definition, and a numpy float32 restatement gives the same bits.  For
 * n = 4^k and a normal v, vm = v / 4^k is exact, so the absolute standard error is 2^-k times statmc_sample_scores' absolute score
 * bit for bit.  Planes that are all 16-byte aligned move four pixels per lane; any other alignment, and the film's last partial
 * group of four, go pixel by pixel to the same bits.
 * STATMC_ERR_INVALID before any launch, statmc_last_error() naming the argument, in this order: a zero width or height; channels not
 * 1 or 3; a metric other than the two; table outside -1..5; with STATMC_SCORE_RELATIVE an eps that is not positive and finite; a NULL
 * or not 4-byte aligned image; score overlapping n, film_mean or film_m2.  STATMC_ERR_NO_DEVICE before statmc_setup, after those
 * checks.  Asynchronous on `stream`: one launch.
 *
 * statmc_plan_to_target: error image + counts so far + tolerance -> count image.  `error` is statmc_error_scores' image, a window of
 * it (statmc_score_window), or the renderer's own metric that falls like 1 / sqrt(n).  n is required.  target is finite and in
 * [2^-60, 2^60]; 0 <= c_min <= c_max <= 2^20.
 * DEFINITION.  The classes of `error` are statmc_plan_samples': saturated e > 2^60, live 2^-60 <= e <= 2^60, dead the rest; n_live
 * and n_saturated count those classes and nothing else.  nn = clamp(n, 0, 2^30).  Per pixel:
 *     saturated, or live with nn < 2 (nobody can judge it):   c = c_max
 *     dead:                                                   c = c_min
 *     live, nn >= 2, e <= target (at the target):             c = c_min
 *     live, nn >= 2, e >  target (open):
 *         r = e / target;  r2 = r * r;  t = r2 * (float)nn;  N = (t >= 2^30) ? 2^30 : (int)ceil(t)
 *         d = max(N - nn, 0);  c = clamp(d, c_min, c_max)
 * At a fixed deviation and quantile the error falls like 1 / sqrt(n): n (e / target)^2 samples in all bring it to the target.  On an
 * open pixel r >= 1, so every intermediate is a normal number or +inf: denormal modes reach no bit, and inf * nn with nn >= 2 is
 * +inf, never NaN.  Hence counts are non-increasing in target; every count lies in [c_min, c_max]; the sums are integer sums, so
 * the same inputs give the same bits on every run; sample_counts is what the counted and compact entries take.
 * One launch behind the zeroing of `result` on `stream` -- a result full of garbage gives the same bits; no workspace, nothing
 * allocated, nothing read back.  `result` is device memory, 8-byte aligned.
 * STATMC_ERR_INVALID before any launch, statmc_last_error() naming the argument, in this order: a zero width or height; NULL error, n,
 * sample_counts or result; error, n or sample_counts not 4-byte aligned, result not 8-byte aligned; a target outside [2^-60, 2^60]
 * (NaN included); c_min / c_max outside 0 <= c_min <= c_max <= 2^20; sample_counts overlapping error, n or result.
 * STATMC_ERR_NO_DEVICE before statmc_setup, after those checks.
 * Measured at 1920 x 1080 and 3840 x 2160: DESIGN.md 4.2g, profiles/error_scores.jsonl. */
#define STATMC_ERROR_NO_TABLE (-1)
int statmc_error_scores(uint16_t width, uint16_t height, int channels, int metric, float eps, int table,
                        const int32_t *n, const float *film_mean, const float *film_m2,
                        float *score, void *stream);

typedef struct statmc_target_result { /* device, written by the call; 48 bytes */
    int64_t total;      /* sum of sample_counts */
    int64_t need;       /* sum over open pixels of max(N - nn, 0), before the clamp: samples still missing, at the present estimates */
    int64_t n_open;     /* judged pixels above the target */
    int64_t n_capped;   /* open pixels whose need exceeds c_max: not reachable in this iteration */
    int64_t n_unjudged; /* saturated pixels, and live ones with fewer than 2 samples */
    int32_t n_live, n_saturated; /* statmc_plan_result's, for the same image */
} statmc_target_result;
int statmc_plan_to_target(uint16_t width, uint16_t height, const float *error, const int32_t *n, float target,
                          int32_t c_min, int32_t c_max, int32_t *sample_counts, statmc_target_result *result,
                          void *stream);

/* ---- order statistics and threshold counts of a score image (no counterpart in the reference): what a stopping rule asks of the
 * error map -- "the 95th percentile of the relative error of the mean is under 2 %", "at most 1 % of the pixels are above tau" --
 * answered on the device, one small struct read back.  `score` is statmc_error_scores' for such a rule (statmc_sample_scores' sample
 * deviation does not fall with the sample count: a threshold on it is never met by rendering more), or the renderer's own metric; a
 * packed width x height plane.
 *
 * DEFINITION.  The key of a score is integer arithmetic on its bit pattern b, so no denormal mode and no comparison instruction
 * reaches a bit:
 *     key(b) = 0   if (b & 0x7FFFFFFF) > 0x7F800000     (NaN, either sign)
 *            = 0   if b has the sign bit                (-0, negatives, -inf)
 *            = b   otherwise                            (+0, subnormals, normals, +inf: bit order is value order)
 * A pixel statmc_plan_samples calls dead through NaN or a negative score sorts with +0.  The classes are statmc_plan_samples',
 * stated on keys:  saturated  key > 0x5D800000 (2^60);  live  0x21800000 <= key <= 0x5D800000;  dead  the rest.
 *
 * statmc_score_select: `ranks` is a HOST array of n_ranks entries, 1 <= n_ranks <= STATMC_SELECT_MAX_RANKS, each in
 * [0, width * height), in any order, repeats allowed.  With sorted_keys the film's keys in non-decreasing order:
 *     value_bits[i] = sorted_keys[rank[i]]          (the rank[i]-th smallest key, 0-based; a float bit pattern, never NaN)
 *     n_below[i]    = the number of pixels with key <  value_bits[i]
 *     n_equal[i]    = the number of pixels with key == value_bits[i]
 * Slots n_ranks .. 7 of the four arrays are written as 0.  Hence n_below[i] <= rank[i] < n_below[i] + n_equal[i], value_bits is
 * non-decreasing in rank, and the same inputs give the same bits on every run: everything is an integer count, so no order
 * reaches a bit.  n_live / n_saturated equal statmc_plan_result's for the same score image.
 * Asynchronous on `stream`; nothing is read back and nothing allocated.  The caller owns `workspace`, at least
 * statmc_score_select_workspace() bytes (a pure function, no device needed) and 8-byte aligned; the call zeroes it on `stream` -- a
 * workspace full of garbage gives the same result -- and leaves nothing of use in it.  `result` is device memory, 8-byte aligned;
 * besides the workspace only `result` is written.  A most-significant-digit radix select on the device: four passes of one 8-bit
 * digit each, every workgroup deriving the prefixes that hold the ranks from the totals of the passes before, then one small
 * launch that writes the result; no kernel waits for another workgroup.
 *
 * statmc_score_count_above: `thresholds` is a HOST array of n_thresholds entries, 1 to 8, none of them NaN;
 *     counts[i] = the number of pixels with key(score_p) > key(thresholds[i])
 * so a negative threshold counts the pixels above +0.  counts is device memory, n_thresholds entries, 8-byte aligned.  One pass over
 * the score image behind the zeroing of counts on `stream`; asynchronous on `stream`.  For a threshold equal to a select's
 * value_bits[i], counts = n_px - n_below[i] - n_equal[i].
 *
 * STATMC_ERR_INVALID before any launch, statmc_last_error() naming the argument, in this order: a zero width or height; NULL score,
 * result / counts, ranks / thresholds or workspace; score not 4-byte aligned; result, counts or workspace not 8-byte aligned;
 * n_ranks / n_thresholds outside 1 to 8; a rank outside the film; a NaN threshold; workspace_bytes below the helper's answer; result
 * or counts overlapping score, result overlapping the workspace, the workspace overlapping score.  STATMC_ERR_NO_DEVICE before
 * statmc_setup, after those checks.
 * Measured at 1920 x 1080 and 3840 x 2160: DESIGN.md 4.2e, profiles/score_select.jsonl. */
#define STATMC_SELECT_MAX_RANKS 8
typedef struct statmc_select_result { /* device, written by the call */
    int64_t n_px, n_live, n_saturated; /* n_live / n_saturated equal statmc_plan_result's for the same score image */
    int32_t n_ranks, pad;
    int64_t rank[STATMC_SELECT_MAX_RANKS];        /* as asked */
    uint32_t value_bits[STATMC_SELECT_MAX_RANKS]; /* key of the rank[i]-th smallest pixel, 0-based: sorted_keys[rank[i]] */
    int64_t n_below[STATMC_SELECT_MAX_RANKS];     /* pixels with key <  value_bits[i] */
    int64_t n_equal[STATMC_SELECT_MAX_RANKS];     /* pixels with key == value_bits[i] */
} statmc_select_result;

size_t statmc_score_select_workspace(void); /* bytes; pure, no device needed */
int statmc_score_select(uint16_t width, uint16_t height, const float *score, const int64_t *ranks, int n_ranks,
                        statmc_select_result *result, void *workspace, size_t workspace_bytes, void *stream);
int statmc_score_count_above(uint16_t width, uint16_t height, const float *score, const float *thresholds, int n_thresholds,
                             int64_t *counts, void *stream);

/* ---- exact sums of a score image (no counterpart in the reference): what a mean or RMS stopping rule asks of the error map --
 * "the mean relative half-width is under 1 %", "the RMS relative error is under T" -- answered on the device with the same bits on
 * every run, one small struct read back.  `score` is what statmc_score_select takes: a packed width x height plane.
 *
 * DEFINITION.  key(b) is statmc_score_select's above: NaN of either sign and everything with the sign bit are 0, the rest their own
 * bit pattern.  For a key k with 0 < k < 0x7F800000:
 *     e = k >> 23,  m = k & 0x7FFFFF,  M = e ? (m | 0x800000) : m,  s = e ? e - 1 : 0
 *     val(k) = M * 2^(s - 149)                          (the float's value, an exact rational);  val(0) = 0
 * `caps` is a HOST array of n_caps entries, 1 <= n_caps <= STATMC_SUM_MAX_CAPS, none of them NaN, in any order, repeats allowed.
 * For cap j, pixel p contributes c = min(key_p, key(caps[j])), taken as unsigned integers (bit order is value order); a pixel whose
 * c is 0x7F800000 is left out of slot j, which is only possible when the cap is +inf: how a caller asks for "no cap".
 *     cap_bits[j]  = key(caps[j])
 *     n_clipped[j] = the number of pixels with key > cap_bits[j]          (statmc_score_count_above's at caps[j])
 *     sum[j]       = the double nearest, ties to even, to the exact sum of val(c) over the pixels
 *     sum_sq[j]    = the double nearest, ties to even, to the exact sum of val(c)^2 over the pixels
 * Neither can overflow or leave a double's normal range: a non-zero one lies in [2^-298, 2^288).  n_zero / n_finite / n_infinite
 * count the pixels by key: == 0; 0 < key < 0x7F800000; == 0x7F800000; they add up to n_px.  Slots n_caps .. 3 of the four arrays
 * are written as 0.  Every quantity is an integer count or the rounding of an integer (a multiple of 2^-149, of 2^-298 for the
 * squares), so the same inputs give the same bits on every run, any permutation of the image gives the same bits, and a
 * restatement in integers of any width is equal bit for bit (tests/score_sum_reference.py).  A mean over the judged pixels is
 * sum / n_px for a finite cap and sum / (n_px - n_infinite) for a cap of +inf; the division is the caller's.
 * Asynchronous on `stream`; nothing is read back and nothing allocated.  The caller owns `workspace`, at least
 * statmc_score_sum_workspace() bytes (a pure function, no device needed) and 8-byte aligned; the call zeroes it on `stream` -- a
 * workspace full of garbage gives the same result -- and leaves nothing of use in it.  `result` is device memory, 8-byte aligned;
 * besides the workspace only `result` is written.  One pass over the image adds every pixel into fixed-point integers of 32-bit
 * limbs held in 64-bit words, one set per interval between the sorted caps; one small launch propagates the carries, forms the
 * capped totals and rounds; no kernel waits for another workgroup.
 *
 * STATMC_ERR_INVALID before any launch, statmc_last_error() naming the argument, in this order: a zero width or height; NULL score,
 * result, caps or workspace; score not 4-byte aligned; result or workspace not 8-byte aligned; n_caps outside 1 to 4; a NaN cap;
 * workspace_bytes below the helper's answer; result overlapping score, result overlapping the workspace, the workspace overlapping
 * score.  STATMC_ERR_NO_DEVICE before statmc_setup, after those checks.
 * Measured at 1920 x 1080 and 3840 x 2160: DESIGN.md 4.2i, profiles/score_sum.jsonl. */
#define STATMC_SUM_MAX_CAPS 4
typedef struct statmc_sum_result { /* device, written by the call */
    int64_t n_px, n_zero, n_finite, n_infinite; /* by key: == 0; 0 < key < 0x7F800000; == 0x7F800000 */
    int32_t n_caps, pad;
    uint32_t cap_bits[STATMC_SUM_MAX_CAPS]; /* key(caps[j]) */
    int64_t n_clipped[STATMC_SUM_MAX_CAPS]; /* pixels with key > cap_bits[j] */
    double sum[STATMC_SUM_MAX_CAPS];
    double sum_sq[STATMC_SUM_MAX_CAPS];
} statmc_sum_result;

size_t statmc_score_sum_workspace(void); /* bytes; pure, no device needed */
int statmc_score_sum(uint16_t width, uint16_t height, const float *score, const float *caps, int n_caps,
                     statmc_sum_result *result, void *workspace, size_t workspace_bytes, void *stream);

/* ---- exact per-tile statistics of a score image (no counterpart in the reference): what a renderer that works tile by tile asks of
 * the error map -- which tiles are still open, how bad the worst tile is, which tiles go on the next iteration's work list -- in one
 * launch.  `score` is what statmc_score_sum takes: a packed width x height plane.
 *
 * DEFINITION.  key(b), val(k), M and s are statmc_score_sum's above.  With T = tile, tiles_x = ceil(width / T) and
 * tiles_y = ceil(height / T), tile (tx, ty) holds the pixels with tx T <= x < min((tx + 1) T, width) and
 * ty T <= y < min((ty + 1) T, height): a partial tile at the right or bottom edge is a tile like any other.  Let ck = key(cap);
 * a cap of +inf means "no cap", as in statmc_score_sum.  Per tile, at entry ty * tiles_x + tx of each plane:
 *     n_px       = the number of pixels of the tile
 *     n_zero     = the number with key == 0;   n_infinite = the number with key == 0x7F800000
 *     n_clipped  = the number with key > ck                                  (statmc_score_count_above's rule at `cap`)
 *     c_p        = min(key_p, ck) as unsigned integers; a pixel whose c_p is 0x7F800000 is left out of the sums, which is only
 *                  possible when ck is: n_counted = n_px - (ck == 0x7F800000 ? n_infinite : 0)
 *     sum        = the double nearest, ties to even, to the exact sum of val(c_p) over the counted pixels; a sum of 0 is +0
 *     sum_sq     = the same of val(c_p)^2
 *     mean       = the float nearest, ties to even, to the exact rational (sum of val(c_p)) / n_counted -- a subnormal result is
 *                  exact in the same way, float's unit 2^-149 being the sums' own --; +0 where n_counted == 0.  It cannot
 *                  overflow: a mean is at most the largest counted value, a finite float
 *     max        = the float whose bit pattern is the maximum of key_p over the tile: not capped, never NaN, never signed
 * Every quantity is an integer count or one rounding of an exact integer or rational: the same inputs give the same bits on every
 * run, any permutation of a tile's pixels gives the same bits, and a restatement in integers of any width is equal bit for bit
 * (tests/score_tiles_reference.py).  `mean` and `max` are tiles_y x tiles_x score images: statmc_score_select,
 * statmc_score_count_above, statmc_score_window and statmc_plan_samples take them as they are; `n_clipped` is a count image that
 * statmc_compact_offsets(..., cap = 1, owners) turns into the list of open tiles.
 * `out` is a HOST struct of DEVICE pointers to packed row-major planes of tiles_y * tiles_x entries; a NULL plane is not formed, at
 * least one is not NULL.  Asynchronous on `stream`: one launch, no workspace, nothing zeroed, nothing allocated, nothing read back,
 * no global atomic; exactly the tiles_x * tiles_y entries of every non-NULL plane are written and nothing else.  A tile belongs to
 * one workgroup (for tile 8 and 16 to part of one wave, to one wave): its pixels are added into fixed-point integers of 32-bit
 * limbs in LDS and the carries, the capped totals, the division and the roundings follow in the same kernel.
 *
 * STATMC_ERR_INVALID before any launch, statmc_last_error() naming the argument, in this order: a zero width or height; NULL score
 * or out; every plane NULL; score not 4-byte aligned; a float or int32_t plane not 4-byte aligned, a double plane not 8-byte
 * aligned; tile not one of 8, 16, 32, 64; a NaN cap; a plane overlapping score or another plane.  STATMC_ERR_NO_DEVICE before
 * statmc_setup, after those checks.
 * Measured at 1920 x 1080 and 3840 x 2160: DESIGN.md 4.2j, profiles/score_tiles.jsonl. */
#define STATMC_SCORE_TILES_MAX_TILE 64
typedef struct statmc_tile_scores { /* HOST struct of DEVICE pointers: packed planes of tiles_y * tiles_x entries, row-major; any may be NULL, not all */
    double *sum, *sum_sq;
    float *mean, *max;
    int32_t *n_px, *n_zero, *n_infinite, *n_clipped;
} statmc_tile_scores;
int statmc_score_tiles(uint16_t width, uint16_t height, const float *score, int tile, float cap,
                       const statmc_tile_scores *out, void *stream);

/* ---- exact per-tile order statistics of a score image, and a per-tile decision brought back to the pixels (no counterpart in the
 * reference): the rule statmc_score_select answers for the film -- "the 95th percentile of the relative half-width is under 2 %" --
 * answered per region in one launch, and the regions that met it closed for good.
 *
 * statmc_score_tile_select.  DEFINITION.  key(b) is statmc_score_select's above; the tile grid is statmc_score_tiles': tile is 8,
 * 16, 32 or 64, tiles_x = ceil(width / tile), tiles_y = ceil(height / tile), a partial tile at the right or bottom edge is a tile like
 * any other.  `q_num` is a HOST array of n_ranks entries, 1 <= n_ranks <= STATMC_TILE_SELECT_MAX_RANKS; 1 <= q_den <= 65536 and
 * 0 <= q_num[i] <= q_den.  For a tile of n pixels (n <= 4096, so n * q_num[i] <= 2^28: integers throughout)
 *     rank_i = max(0, ceil(n * q_num[i] / q_den) - 1)
 * the nearest-rank rule (Estimator::NearestRank) for q = q_num[i] / q_den: q = 1 is the tile's maximum, q = 0 its minimum, 1/2 the
 * lower median.  With sorted the tile's keys in non-decreasing order, at entry ty * tiles_x + tx of the planes of slot i:
 *     value[i]   = the float whose bit pattern is sorted[rank_i]: never NaN, never signed
 *     n_below[i] = the number of the tile's pixels with key <  that value
 *     n_equal[i] = the number of the tile's pixels with key == that value
 * so n_below[i] <= rank_i < n_below[i] + n_equal[i].  +inf pixels are counted like any other and sort on top: a tile of pixels nobody
 * can judge yet stays open under every finite threshold.  Everything is an integer count or a bit pattern found by counting: the same
 * inputs give the same bits on every run, any permutation of a tile's pixels gives the same bits, and np.sort of the keys per tile
 * is equal bit for bit (tests/tile_select_reference.py).  The `value` planes are tiles_y x tiles_x score images:
 * statmc_score_count_above, statmc_score_select, statmc_score_window, statmc_plan_samples and statmc_gate_tiles take them as they
 * are; value at q = 1 is statmc_score_tiles' max.
 * `out` is a HOST struct of DEVICE pointers to packed row-major planes of tiles_y * tiles_x entries.  Any plane may be NULL and is
 * then not formed; at least one plane is not NULL, and every plane of the slots n_ranks .. 3 is NULL.  Asynchronous on `stream`: one
 * launch, no workspace, nothing zeroed, nothing allocated, nothing read back, no global atomic; exactly the tiles_x * tiles_y entries
 * of every non-NULL plane are written and nothing else.  A tile belongs to 16 lanes (tile 8), a wave (16) or a workgroup (32, 64);
 * its keys stay in registers and all ranks descend together over the 31 key bits, one count per bit.
 *
 * STATMC_ERR_INVALID before any launch, statmc_last_error() naming the argument, in this order: a zero width or height; NULL score,
 * q_num or out; every plane NULL, or -- for n_ranks in 1 .. 4 -- a plane in a slot >= n_ranks; score not 4-byte aligned; a plane not
 * 4-byte aligned; tile not one of 8, 16, 32, 64; n_ranks outside 1 .. 4; q_den outside 1 .. 65536; a q_num[i] outside 0 .. q_den; a
 * plane overlapping score or another plane.  STATMC_ERR_NO_DEVICE before statmc_setup, after those checks.
 *
 * statmc_gate_tiles.  DEFINITION.  `tile_value`, `closed` and `open` are planes of the same tile grid.  Per tile t:
 *     was_closed = closed != NULL && closed[t] != 0
 *     above      = key(tile_value[t]) > key(threshold)        (statmc_score_count_above's rule; a NaN threshold is refused)
 *     open[t]    = !was_closed && above ? 1 : 0
 *     closed[t]  = was_closed ? as it was : (above ? 0 : 1)    (only if closed is given)
 * A closed tile never reopens; a caller starts from a plane zeroed with statmc_memset.  `result`, if given, is device memory, 8-byte
 * aligned: n_tiles; n_open = the number of tiles with open[t] == 1; n_closed_now = the number with !was_closed && !above;
 * n_px_open = the number of pixels of the open tiles, from the grid's geometry.  `src` and `dst` are HOST arrays of n_images,
 * 0 <= n_images <= STATMC_GATE_MAX_IMAGES, device images of width x height 32-bit words; per image i and pixel p, as words,
 *     dst_i[p] = open[tile of p] ? src_i[p] : 0
 * The all-zero word is +0 of a score image and 0 of a count image: one entry gates both.  A score image gated before
 * statmc_plan_samples sends the budget to the open tiles (with c_min = 0 a closed pixel gets nothing); a count image gated after
 * the plan is exactly 0 in closed tiles whatever c_min was, and statmc_compact_offsets gives the new total.  dst_i may be exactly
 * src_i (in place).  `open` is the count image that statmc_compact_offsets(tiles_x, tiles_y, ..., cap = 1, owners) turns into the
 * list of open tiles.  Asynchronous on `stream`, nothing read back, nothing allocated: `result` is zeroed on the stream; a tile pass
 * decides, updates closed -- each word read and written by one lane only -- and writes open and, one 64-bit atomic per workgroup and
 * count, the result; a pixel pass (not launched for n_images == 0) moves aligned quads of all images at once.
 *
 * STATMC_ERR_INVALID before any launch, statmc_last_error() naming the argument, in this order: a zero width or height; NULL
 * tile_value or open; n_images outside 0 .. 4; with n_images > 0, NULL src or dst, then a NULL src[i] or dst[i]; tile_value, closed,
 * open, a src[i] or a dst[i] not 4-byte aligned; result not 8-byte aligned; tile not one of 8, 16, 32, 64; a NaN threshold; overlaps:
 * of two of tile_value, closed, open and result; of src[i] and dst[i] unless they are equal; of an image with tile_value, closed,
 * open or result; of dst[i] with src[j] or dst[j], j != i.  STATMC_ERR_NO_DEVICE before statmc_setup, after those checks.
 * Measured at 1920 x 1080 and 3840 x 2160: DESIGN.md 4.2k, profiles/score_tile_select.jsonl. */
#define STATMC_TILE_SELECT_MAX_RANKS 4
#define STATMC_GATE_MAX_IMAGES 4
typedef struct statmc_tile_quantiles { /* HOST struct of DEVICE pointers: packed tiles_y x tiles_x planes, row-major */
    float *value[STATMC_TILE_SELECT_MAX_RANKS];
    int32_t *n_below[STATMC_TILE_SELECT_MAX_RANKS];
    int32_t *n_equal[STATMC_TILE_SELECT_MAX_RANKS];
} statmc_tile_quantiles;
int statmc_score_tile_select(uint16_t width, uint16_t height, const float *score, int tile,
                             const int32_t *q_num, int32_t q_den, int n_ranks,
                             const statmc_tile_quantiles *out, void *stream);
typedef struct statmc_gate_result { int64_t n_tiles, n_open, n_closed_now, n_px_open; } statmc_gate_result; /* device, 8-byte aligned */
int statmc_gate_tiles(uint16_t width, uint16_t height, int tile,
                      const float *tile_value, float threshold,
                      int32_t *closed,              /* in/out tiles plane, may be NULL */
                      int32_t *open,                /* out tiles plane, required */
                      const void *const *src, void *const *dst, int n_images,   /* HOST arrays, 0..4 device images of width x height 32-bit words */
                      statmc_gate_result *result,   /* may be NULL */
                      void *stream);

/* ---- window maximum / minimum of a score image (no counterpart in the reference): the error map regularised over a neighbourhood
 * before a plan spends by it.  A pixel's sample standard deviation after a handful of samples is itself noisy: a pixel beside a
 * caustic that has not yet drawn a bright sample reports a small score and the plan starves it.  MAX gives every pixel the worst
 * score within `radius` pixels (a dilation); MIN then MAX with the same radius (an opening) removes isolated spikes first.
 *
 * DEFINITION.  key(b) is statmc_score_select's above: NaN of either sign and everything with the sign bit are 0, the rest their own
 * bit pattern.  The window of pixel (x, y) is the pixels (x', y') of the film with |x' - x| <= radius and |y' - y| <= radius: taps
 * outside the film are skipped (the border is clipped), the centre is always a member.
 *     out[y][x] = the float whose bit pattern is the maximum (op STATMC_SCORE_WINDOW_MAX) or the minimum (STATMC_SCORE_WINDOW_MIN),
 *                 as unsigned integers, of key(score[y'][x']) over the window.
 * Hence the output is never NaN and never has the sign bit; radius 0 canonicalises an image (the identity on non-negative, non-NaN
 * scores); the same inputs give the same bits on every run (integer maxima: no order reaches a bit); window(op, r2) of
 * window(op, r1) equals window(op, r1 + r2) bit for bit, clipped borders included; on a non-negative, non-NaN image MAX is a
 * (2 radius + 1)^2 max-pooling with stride 1 and implicit -inf padding, bit for bit.  The classes statmc_plan_samples and
 * statmc_score_select assign are those of the output's keys: `out` is what both take as `score`.
 * Asynchronous on `stream`: one launch, no workspace, nothing allocated, nothing read back; only `out` is written, exactly its
 * width * height floats.  A workgroup stages a tile and its halo as keys in LDS, reduces along rows, then along columns, each by
 * doubling -- log2(2 radius + 1) steps, not 2 radius + 1 taps.
 *
 * STATMC_ERR_INVALID before any launch, statmc_last_error() naming the argument, in this order: a zero width or height; NULL score
 * or out; score or out not 4-byte aligned; op not one of the two; radius outside [0, STATMC_SCORE_WINDOW_MAX_RADIUS]; out
 * overlapping score (there is no in-place mode).  STATMC_ERR_NO_DEVICE before statmc_setup, after those checks.
 * Measured at 1920 x 1080 and 3840 x 2160: DESIGN.md 4.2f, profiles/score_window.jsonl. */
#define STATMC_SCORE_WINDOW_MAX 0
#define STATMC_SCORE_WINDOW_MIN 1
#define STATMC_SCORE_WINDOW_MAX_RADIUS 32
int statmc_score_window(uint16_t width, uint16_t height, const float *score, int op, int radius,
                        float *out, void *stream);

/* ---- the compact arena of a planned iteration: every pixel's samples back to back, pixels in raster order (CSR).  Pixel p owns
 * positions [offsets[p], offsets[p + 1]) of a sample-major [total][channels] array per stat type: no pixel index per sample, no
 * sort, no dead slots, `total` samples of memory.  The loop: statmc_plan_samples -> statmc_compact_offsets -> the renderer writes
 * pixel p's sample s at position offsets[p] + s -> statmc_compact_accumulate.
 *
 * statmc_compact_offsets: count image -> offsets, and optionally owners.
 *     c(p) = min(max(sample_counts[p], 0), cap),  cap >= 0, INT32_MAX: no cap
 *     offsets[p] = the sum of c(q) over q < p in raster order, int64, p = 0 .. width * height; offsets[width * height] is the total.
 *     owners != NULL:  owners[i] = p for offsets[p] <= i < min(offsets[p + 1], owners_capacity), -1 for every i in
 *                      [total, owners_capacity).
 * Every sum is an integer sum: the same bits on every run.  The total stays on the device; nothing is read back, nothing is
 * allocated.  owners is a valid pixels[] of the records entries (-1: a skipped record) and the slot-to-pixel map of a renderer that
 * runs one thread per sample.  Three launches like statmc_plan_samples' trim (block sums, one workgroup over them, apply) and one
 * more over the owner slots; no kernel waits for another workgroup.  The caller owns `workspace`, at least
 * statmc_compact_offsets_workspace(width, height) bytes (pure, no device needed; a multiple of 8, monotone in the pixel count) and
 * 8-byte aligned.
 * STATMC_ERR_INVALID before any launch, statmc_last_error() naming the argument: a zero width or height; NULL sample_counts, offsets
 * or workspace; sample_counts or owners not 4-byte aligned, offsets or workspace not 8-byte aligned; cap < 0; owners_capacity < 0,
 * or non-zero with NULL owners; workspace_bytes below the helper's answer; offsets or owners overlapping sample_counts, the
 * workspace or each other.  STATMC_ERR_NO_DEVICE before statmc_setup, after those checks.  Asynchronous on `stream`. */
size_t statmc_compact_offsets_workspace(uint16_t width, uint16_t height); /* bytes; pure, no device needed */
int statmc_compact_offsets(uint16_t width, uint16_t height, const int32_t *sample_counts, int32_t cap,
                           int64_t *offsets, int32_t *owners, int64_t owners_capacity,
                           void *workspace, size_t workspace_bytes, void *stream);

/* statmc_compact_accumulate: the fold of a compact arena.  types[t].samples is sample-major [n_samples][channels], fp32 or IEEE half
 * as sample_formats[t] says (STATMC_SAMPLES_F32 / STATMC_SAMPLES_F16; NULL: every type fp32); n_samples is the arena's length in
 * samples, given by the host who sized it; types[t].n_samples is ignored.
 * DEFINITION, per pixel p:  start = clamp(offsets[p], 0, n_samples),  end = clamp(offsets[p + 1], start, n_samples),  c = end - start.
 * The clamp comes before anything is derived from an offset: no value of offsets[], however wrong, becomes an address outside
 * [0, n_samples).  Apart from that, non-monotone or out-of-range offsets have no defined result.
 *   c <= split_above  the pixel holds, bit for bit, what statmc_accumulate_records leaves for samples start .. end - 1 in that
 *                     order, half samples widened first: n, every moment, the film chain and the mean_corr / discriminator
 *                     epilogue where asked.  c == 0 keeps every bit of every image.
 *   c >  split_above  the pixel holds, bit for bit, what statmc_accumulate_records_split leaves for that run: 64 chunks of
 *                     ceil(c / 64) samples, slot 0 continuing the stored state, merged by the fixed tree of merge_lanes<64>.
 *                     split_above < 1 is refused; INT32_MAX: never split; STATMC_RECORDS_SPLIT_DEFAULT is the documented choice.
 * Hence: the call equals the records entries on (owners, samples) of statmc_compact_offsets, bit for bit; the same inputs give the
 * same bits on every run; the call is asynchronous on `stream`, reads nothing back and allocates nothing -- no workspace, no sort.
 * Positions are 64-bit throughout: there is no 2^31 limit on n_samples (a 4K film at 256 spp has 2.1 G samples).  A pixel's count
 * stays below 2^24, as everywhere else.
 * STATMC_ERR_INVALID before any launch, statmc_last_error() naming the argument: n_types outside [0, 16]; NULL types or offsets
 * with work to do; n_samples < 0; a sample format other than the two; a half arena at an odd address; an fp32 arena not 4-byte or
 * offsets not 8-byte aligned; split_above < 1.  STATMC_ERR_NO_DEVICE before statmc_setup, after those checks; then a zero width or
 * height and the descriptors' own rules (statmc_accumulate_records').  Zero types or zero samples is a no-op.
 * Measured at 1920 x 1080: DESIGN.md 4.1j, profiles/accumulate_compact.jsonl. */
int statmc_compact_accumulate(uint16_t width, uint16_t height, const statmc_stat_type *types, const int32_t *sample_formats,
                              int n_types, const int64_t *offsets, int64_t n_samples, int32_t split_above, void *stream);

/* statmc_compact_accumulate_interleaved: the fold of a compact arena of interleaved records -- ONE array, record i at
 * (char *)records + i * layout->stride, holding every type's values: the struct a renderer with one thread per planned sample
 * stores at slot offsets[p] + s.  layout->stride, sample_offset[t] and sample_format[t] mean what they mean for
 * statmc_accumulate_records_interleaved and obey its rules: the stride a multiple of 4 and at least 4; an offset a multiple of the
 * element size with the field inside the stride; fields in any order, padded or overlapping; records 4-byte aligned.
 * layout->pixel_offset is neither read nor checked: a compact record needs no pixel field.  types[t].samples and
 * types[t].n_samples are ignored.  Positions and byte offsets are 64-bit throughout: n_records has no 2^31 limit.
 * DEFINITION, per pixel p:  start = clamp(offsets[p], 0, n_records),  end = clamp(offsets[p + 1], start, n_records), clamped before
 * anything is derived from them.  The call leaves, bit for bit, what statmc_compact_accumulate leaves when it gets the same offsets
 * and split_above, n_samples = n_records, and as type t's arena the [n_records][channels] array of every record's field t in that
 * field's format.  Hence it equals statmc_accumulate_records on the same samples, statmc_accumulate_records_split above
 * split_above, and statmc_accumulate_records_interleaved[_split] on the same records with the owners written into a pixel field;
 * and everything statmc_compact_accumulate promises carries over: c == 0 keeps every bit, the stored state is continued, the
 * pre-pass epilogue runs where a type has mean_corr / discriminator, the same inputs give the same bits on every run, the call is
 * asynchronous on `stream`, reads nothing back and allocates nothing -- no workspace, no sort --, and no value of offsets[] becomes
 * an address outside [records, records + n_records * stride).
 * One lane per pixel folds every stat type from one read of each record where the type set is one of the fused records fold's
 * (one RGB type with the transform and three moments, up to two mean-only RGB and up to two mean-only 1-channel types, every field
 * fp32 or the feature fields half); every other valid call is served by one lane per pixel and type.  Runs above split_above are
 * folded by the 64 lanes of a wave in a launch of their own behind the fused one.
 * STATMC_ERR_INVALID before any launch, statmc_last_error() naming the argument: n_types outside [0, 16]; NULL types, layout,
 * records or offsets with work to do; n_records < 0; a stride, records address, sample format, channel count (1 or 3) or sample
 * offset outside the rules; offsets not 8-byte aligned; split_above < 1.  STATMC_ERR_NO_DEVICE before statmc_setup, after those
 * checks; then a zero width or height and the descriptors' own rules.  Zero types or zero records is a no-op.
 * Measured at 1920 x 1080: DESIGN.md 4.1k, profiles/accumulate_compact_interleaved.jsonl. */
int statmc_compact_accumulate_interleaved(uint16_t width, uint16_t height, const statmc_stat_type *types, int n_types,
                                          const void *records, const statmc_record_layout *layout,
                                          const int64_t *offsets, int64_t n_records, int32_t split_above, void *stream);

/* ---- the state of a pixel as a thing that travels: unordered (pixel, state) records.  The dense entries put whole films together
 * (statmc_combine_statistics, statmc_combine_many, statmc_pool_statistics); these two move the states of LISTED pixels, any number in
 * any order.  Who needs them: a wavefront renderer whose waves fold a pixel's samples in registers
 * (statmc::device::PixelStats) without owning the pixel -- it writes one record per (wave, pixel) with PixelStats::write_record
 * instead of one sample record per sample --, and a helper device that re-rendered a few per cent of a film and ships those
 * pixels' states instead of whole images.
 *
 * THE STATE RECORD of a stat type with C channels, max_moment M and the transform flag is D = 1 + C * (M + (transform ? 2 : 0))
 * dwords: dword 0 the int32 count n, then per channel mean, m2 (M >= 2), m3 (M = 3), film_mean, film_m2 (transform types only),
 * every float as its bits -- the order of statmc::device::map_state (include/statmc_device_api.hpp), which PixelStats::write_record /
 * read_record write and read.  D = 16 for the radiance type (3 channels, transform, M = 3), 4 for normal / albedo, 2 for a mean-only
 * 1-channel type.  statmc_state_dwords returns D; it is pure, needs no device and returns 0 for values a stat type cannot have
 * (channels other than 1 and 3, max_moment outside 1 .. 3).  It agrees with statmc::device::state_dwords<C, MAXM, TRANSFORM>().
 * states is a HOST array of n_types DEVICE pointers; states[t] is record-major [n_records][D_t] dwords, 4-byte aligned.
 *
 * statmc_gather_states: record i of type t receives, bit for bit, the stored state of pixel pixels[i].  A pixel value outside
 * [0, width * height) gets the state of no samples -- n = 0, every field +0 -- and never becomes an address.  Duplicates are fine;
 * the images are only read.  types[t].samples, n_samples, mean_corr and discriminator are ignored.  No workspace.
 *
 * statmc_combine_records: DEFINITION, per pixel p and type t.  The run of p is the records of this call with pixels[i] == p, in
 * ascending i; c is its length.  A record whose count for type t is <= 0 carries nothing for that type and is passed over: no field
 * of it is read into any formula.
 *   c <= split_above  start from the stored state S; for each record R_i of the run in order with n_i > 0, S.merge(R_i) with S as
 *                     part A and the record as part B: bit for bit a chain of two-part statmc_combine_statistics calls in that
 *                     order, and the left fold statmc_combine_many computes from the same parts.
 *   c >  split_above  the run is cut into STATMC_RECORDS_SPLIT_LANES chunks of ceil(c / 64) records, a function of c alone (the
 *                     chunk rule of statmc_accumulate_records_split); slot 0 starts from the stored state, every slot j > 0 from
 *                     the state of no samples; each slot left-folds its chunk as above; the 64 states are merged in the tree of
 *                     merge_lanes<64> (include/statmc_device_api.hpp): the relation statmc_accumulate_records_split has to
 *                     statmc_accumulate_records.  split_above >= 1; INT32_MAX: never split.
 * A pixel and type with at least one record of positive count is stored, its pre-pass to mean_corr / discriminator where the type
 * has them (max_moment 3).  Every other pixel keeps every bit of every image, mean_corr / discriminator included.
 * Hence, as for the records entries: a dead pixel value never becomes an address; the result does not depend on how records of
 * different pixels interleave; without a split, a call over [0, n) equals calls over [0, m) and [m, n); the same inputs give the
 * same bits on every run.  The grouping is the stable sort of statmc_accumulate_records, in the same per-(device, stream)
 * workspace.  Every type carries its own n (no borrowed counts); the counts of a pixel sum below 2^24.  types[t].samples and
 * n_samples are ignored.
 *
 * Both calls are asynchronous on `stream` and read nothing back.  STATMC_ERR_INVALID before any launch, statmc_last_error() naming
 * the argument: n_types outside [0, 16]; n_records outside [0, 2^31); split_above < 1; then, with work to do, NULL types, pixels or
 * states, pixels or a states[t] NULL or not 4-byte aligned, a zero width or height, and the descriptors' own rules
 * (statmc_accumulate_records').  Zero types or zero records is a no-op.  STATMC_ERR_NO_DEVICE before statmc_setup, after those checks.
 * Measured at 1920 x 1080: DESIGN.md 4.2d, profiles/combine_records.jsonl. */
size_t statmc_state_dwords(int channels, int max_moment, int transform); /* dwords; pure, no device needed */
int statmc_gather_states(uint16_t width, uint16_t height, const statmc_stat_type *types, int n_types,
                         const int32_t *pixels, int64_t n_records, void *const *states, void *stream);
int statmc_combine_records(uint16_t width, uint16_t height, const statmc_stat_type *types, int n_types,
                           const int32_t *pixels, int64_t n_records, const void *const *states,
                           int32_t split_above, void *stream);

/* Scatter of reference-layout AoS tiles (StatTilePixel<T>, estimator.h:104-124: 64 B for
 * T=float, 128 B for T=Vec3) that were accumulated on the host into the planar device images:
 * Estimator::MergeTile / MergeTransformTile.  tile_bounds = {x0,y0,x1,y1} per tile (device,
 * int32 x4), tile_offsets = index of each tile's first pixel in tile_pixels (device), in any order.  n takes the low 32 bits of
 * the 64-bit count, every other field is copied bit for bit; pixels no tile covers, and without `transform` the film images
 * (which may then be null), are left as they are.  max_tile_pixels sizes the launch -- the pixel count of the largest tile is the
 * value to pass -- and a tile with more pixels than that is still scattered whole.  At most 65535 tiles per call: more are
 * refused with STATMC_ERR_UNSUPPORTED and nothing is written. */
int statmc_merge_tiles(uint16_t width, uint16_t height, int channels, int transform,
                       const void *tile_pixels, const int32_t *tile_bounds,
                       const int64_t *tile_offsets, int n_tiles, int max_tile_pixels,
                       int32_t *n, float *mean, float *m2, float *m3, float *film_mean,
                       float *film_m2, void *stream);

/* Film::UpdateImage on the device (src/core/film.cpp:188-222): reads the reference's AoS
 * Film::Pixel array {float xyz[3]; float filterWeightSum; float splatXYZ[3]; float pad} (32 B per
 * pixel, src/core/film.h:72-78) and writes the interleaved RGB "film" image the filter denoises:
 * XYZ -> RGB, / weight sum, clamp >= 0, + splat_scale * splat RGB, * scale. */
int statmc_film_update(const void *film_pixels, size_t n_pixels, float splat_scale, float scale, float *film_rgb,
                       void *stream);

/* Tile-local pooled moments of an image by wavefront-level Welford/Chan merges: for every
 * tile_size x tile_size tile writes {count, mean, M2} per channel of `values`
 * (out: [tiles_y][tiles_x][channels][3] fp32).  tile_size in {8, 16}. */
int statmc_tile_moments(uint16_t width, uint16_t height, int channels, const float *values,
                        int tile_size, float *out, void *stream);

/* Introspection used by tests/bench: name of the window-filter kernel variant the last
 * statmc_window_filter call dispatched ("lds_r20", "lds_rt", "generic", ...). */
const char *statmc_last_filter_variant(void);
int statmc_version(void);

/* Measurement aid (bench.py "shader_clock"; no counterpart in the reference): one wave counts `cycles` shader clocks
 * (s_memtime) against the constant 100 MHz clock (s_memrealtime) and writes {shader clocks, 10 ns ticks} to
 * out[0..1] (device, int64).  Enqueued right behind a kernel it reports the clock the power manager held for that
 * kernel.  The loop ends after `cycles` shader clocks (1 .. 2^24). */
int statmc_clock_probe(int64_t *out, int cycles, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* STATMC_H */
