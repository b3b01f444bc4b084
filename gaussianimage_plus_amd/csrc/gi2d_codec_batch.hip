// Several pictures per decode launch (include/gi2d.h "batched decode"; DESIGN.md 3.8 "Batches"): what gi2d_batch.h does
// for the fitting kernels, for the decoder.  One picture of a few thousand gaussians is a handful of decode workgroups
// and at most one residency round of tile workgroups walking the same phases in lockstep, and its three launches cost
// as much host time as they run; K pictures per launch overlap each other's latency and share the launches.
//
//   table     head (the workgroup index at which picture k starts, per kernel) + one argument block per picture, written
//             by kernels that carry the blocks as kernel arguments (gi2d_train.hip::write_batch_table has the reasons)
//   reset     every workspace as gi2d_fast_workspace_init leaves what a decode reads of it
//   decode    gi2d_codec_core.h::codec_decode_bin_one, 256 gaussians per workgroup; kind and view are per picture: a
//             workgroup-uniform switch over the four instantiations the single-picture launch chooses from on the host
//   draw      gi2d_codec_core.h::codec_draw_tile on the picture's own lists, records, status row and slice of `out`
//   affine    a call with an affine picture among its K (gi2d_codec_decode_batch_affine) launches the AFFINE = true
//             instantiation of the two kernels: the decode switch has the two affine forms as well, and the draw picks per
//             picture between codec_draw_tile and codec_draw_tile_rows (one LDS block serves either).  The maps travel in
//             a table of their own behind the argument blocks; the AFFINE = false instantiations, which a call without an
//             affine picture launches, neither read that table nor reserve the whole-row draw's LDS.
//
// A workgroup finds its picture with batch_find and touches that picture's workspace and status row only, so every
// access rule of gi2d_fast_internal.h holds per workspace exactly as in the single-picture launches, and nothing is
// handed from one workgroup to another inside a launch.
#include <string>
#include <vector>

#include "gi2d_batch.h"
#include "gi2d_codec_core.h"

namespace gi2d {

struct CodecBatchPicture {
    CodecLayout lay;
    CodecSide side;
    const uint32_t *payload;
    long long last_dword;
    int n, form;  // form: (kind == scale-rot) * 2 + view; affine: 4 + (kind == scale-rot), its map in the affine table
    float clip_coe, radius_clip;
    CodecView vw;
    BinTarget bt;  // prev_box, lists, record sets and the status row (colour comes from the record, opacity is 1)
    int2 *tile_bins;
    void *out;
};
struct CodecBatchHead {
    int pg_start[96];    // decode/bin workgroup at which picture k starts; entry K = total (GI2D_BATCH_MAX + 1 used)
    int tile_start[96];  // the same for the draw kernel
};
struct CodecBatchTable {
    CodecBatchHead *head;
    CodecBatchPicture *pic;
    CodecAffine *affine;  // [k]: entry i is read by the workgroups of picture i when its form is an affine one
    size_t bytes;
};
static inline CodecBatchTable carve_codec_batch(void *base, int k) {
    CodecBatchTable b;
    const size_t kk = (size_t)(k > 0 ? k : 1);
    b.head = (CodecBatchHead *)base;
    b.pic = (CodecBatchPicture *)((char *)base + align_up(sizeof(CodecBatchHead)));
    b.affine = (CodecAffine *)((char *)b.pic + align_up(kk * sizeof(CodecBatchPicture)));
    b.bytes = align_up(sizeof(CodecBatchHead)) + align_up(kk * sizeof(CodecBatchPicture)) + align_up(kk * sizeof(CodecAffine));
    return b;
}

#define GI2D_CODEC_BATCH_PACK 14 /* argument blocks per writer launch (kernel arguments are limited to 4 KB) */
struct CodecBatchPack {
    CodecBatchPicture pic[GI2D_CODEC_BATCH_PACK];
};
struct CodecBatchAffines {
    CodecAffine af[GI2D_BATCH_MAX];
};
static_assert(sizeof(CodecBatchPack) <= 3840 && sizeof(CodecBatchHead) <= 3840 && sizeof(CodecBatchAffines) <= 3840,
              "a writer's block must fit the kernel-argument segment");  // (gi2d_batch.h::codec_batch_write_kernel)

// What gi2d_fast.hip::fast_ws_init_kernel resets of the regions a decode workspace has (carve_decode): the version words,
// the pool cursor, every row header, every previous box.  blocks_per_picture * 256 lanes per picture.
__global__ __launch_bounds__(256) void codec_reset_batched_kernel(const CodecBatchPicture *__restrict__ pics,
                                                                  int blocks_per_picture, int num_tiles) {
    const int k = (int)blockIdx.x / blocks_per_picture;
    const int i = ((int)blockIdx.x - k * blocks_per_picture) * 256 + (int)threadIdx.x;
    const CodecBatchPicture &p = pics[k];
    int32_t *lists = p.bt.lists;
    if (i < GI2D_VER_WORDS) p.bt.recs.ver[i] = 0;
    if (i == 0) lists[GI2D_POOL_CURSOR] = 0;
    if (i < num_tiles) {
        lists[(size_t)i * GI2D_FAST_LROW] = 0;
        lists[(size_t)i * GI2D_FAST_LROW + 1] = 0;
    }
    if (i < p.n) p.bt.prev_box[i] = no_box();
}

template <bool AFFINE>
__global__ __launch_bounds__(256) void codec_decode_bin_batched_kernel(const CodecBatchHead *__restrict__ head,
                                                                       const CodecBatchPicture *__restrict__ pics,
                                                                       const CodecAffine *__restrict__ affines,
                                                                       int k_pictures, float img_w, float img_h,
                                                                       int tiles_x, int tiles_y) {
    const int k = batch_find(head->pg_start, k_pictures, (int)blockIdx.x);
    const CodecBatchPicture &p = pics[k];
    const int g = ((int)blockIdx.x - head->pg_start[k]) * 256 + (int)threadIdx.x;
    const CodecOut none{nullptr, nullptr, nullptr, nullptr, nullptr};
#define GI2D_DECODE_ONE(KIND, FORM)                                                                                     \
    codec_decode_bin_one<KIND, FORM>(g, p.n, p.lay, p.side, p.payload, p.last_dword, p.clip_coe, img_w, img_h, tiles_x, \
                                     tiles_y, p.radius_clip, none, p.bt, p.vw, af)
    CodecAffine af{};
    if constexpr (AFFINE) af = affines[k];
    if constexpr (AFFINE) {  // (a case label cannot stand inside an `if constexpr` of its switch: two switches)
        switch (p.form) {    // workgroup-uniform
            case 0: GI2D_DECODE_ONE(kCovariance, GI2D_CODEC_FORM_FULL); break;
            case 1: GI2D_DECODE_ONE(kCovariance, GI2D_CODEC_FORM_VIEW); break;
            case 2: GI2D_DECODE_ONE(kScaleRot, GI2D_CODEC_FORM_FULL); break;
            case 3: GI2D_DECODE_ONE(kScaleRot, GI2D_CODEC_FORM_VIEW); break;
            case 4: GI2D_DECODE_ONE(kCovariance, GI2D_CODEC_FORM_AFFINE); break;
            default: GI2D_DECODE_ONE(kScaleRot, GI2D_CODEC_FORM_AFFINE); break;
        }
    } else {
        switch (p.form) {
            case 0: GI2D_DECODE_ONE(kCovariance, GI2D_CODEC_FORM_FULL); break;
            case 1: GI2D_DECODE_ONE(kCovariance, GI2D_CODEC_FORM_VIEW); break;
            case 2: GI2D_DECODE_ONE(kScaleRot, GI2D_CODEC_FORM_FULL); break;
            default: GI2D_DECODE_ONE(kScaleRot, GI2D_CODEC_FORM_VIEW); break;
        }
    }
#undef GI2D_DECODE_ONE
}

// AFFINE: the draw routine is the picture's (workgroup-uniform), and the LDS block is large enough for either
template <bool AFFINE, int DTYPE, int LAYOUT>
__global__ __launch_bounds__(256) void codec_draw_batched_kernel(const CodecBatchHead *__restrict__ head,
                                                                 const CodecBatchPicture *__restrict__ pics,
                                                                 int k_pictures, int tiles_x, int tiles_y, int img_w,
                                                                 int img_h, const float *__restrict__ background) {
    constexpr size_t LDS = AFFINE && sizeof(RowsLds) > sizeof(FwdLds) ? sizeof(RowsLds) : sizeof(FwdLds);
    __shared__ __align__(16) unsigned char lds[LDS];
    __shared__ int grp[32];
    const int k = batch_find(head->tile_start, k_pictures, (int)blockIdx.x);
    const CodecBatchPicture &p = pics[k];
    const int tile = (int)blockIdx.x - head->tile_start[k];
    if constexpr (AFFINE) {
        if (p.form >= 4) {
            codec_draw_tile_rows<DTYPE, LAYOUT>(*reinterpret_cast<RowsLds *>(lds), grp, tile, tile == 0, tiles_x, tiles_y,
                                                img_w, img_h, p.bt.recs, background, p.bt.lists, p.tile_bins, p.bt.status,
                                                p.out);
            return;
        }
    }
    codec_draw_tile<DTYPE, LAYOUT>(*reinterpret_cast<FwdLds *>(lds), grp, tile, tile == 0, tiles_x, tiles_y, img_w, img_h,
                                   p.bt.recs, background, p.bt.lists, p.tile_bins, nullptr, nullptr, p.bt.status, p.out);
}

static inline size_t pixel_plane_bytes(int dtype, int layout, size_t h, size_t w_) {
    const size_t elem = dtype == GI2D_PIXEL_F32 ? 4 : dtype == GI2D_PIXEL_F16 ? 2 : 1;
    return h * w_ * (layout == GI2D_LAYOUT_HWC4 ? 4 : 3) * elem;
}

}  // namespace gi2d

using namespace gi2d;

extern "C" {

size_t gi2d_codec_batch_bytes(int num_pictures) { return carve_codec_batch(nullptr, num_pictures).bytes; }

size_t gi2d_codec_decode_workspace_bytes(int n, int tiles_x, int tiles_y) {
    if (n < 0 || tiles_x < 0 || tiles_y < 0 || (long long)tiles_x * tiles_y > 0x7fffffffLL) return 0;
    return carve_decode(nullptr, n, tiles_x * tiles_y).bytes;
}

int gi2d_codec_decode_batch(int num_pictures, const gi2d_codec_picture *pictures, void *batch, size_t batch_bytes,
                            unsigned out_h, unsigned out_w, int tiles_x, int tiles_y, const float *background, int dtype,
                            int layout, void *out, gi2d_stream_t st) {
    return gi2d_codec_decode_batch_affine(num_pictures, pictures, nullptr, batch, batch_bytes, out_h, out_w, tiles_x, tiles_y,
                                          background, dtype, layout, out, st);
}

int gi2d_codec_decode_batch_affine(int num_pictures, const gi2d_codec_picture *pictures, const gi2d_codec_affine *affines,
                                   void *batch, size_t batch_bytes, unsigned out_h, unsigned out_w, int tiles_x,
                                   int tiles_y, const float *background, int dtype, int layout, void *out,
                                   gi2d_stream_t st) {
    const auto fail = [&](const std::string &why) {
        set_error(("codec decode batch: " + why).c_str());
        return GI2D_ERR_INVALID_ARGUMENT;
    };
    // ---- everything is checked before anything is launched (and before any device call at all)
    if (num_pictures < 1 || num_pictures > GI2D_BATCH_MAX) return fail("1 .. 64 pictures per call");
    if (!pictures || !batch || !out) return fail("null pointer");
    if (!pixel_format_ok(dtype, layout)) return fail("unknown picture format (dtype 0..2, layout 0..2)");
    if (out_h < 1 || out_w < 1) return fail("empty output");
    if (tiles_x < 1 || tiles_y < 1 || (long long)tiles_x * GI2D_TILE < (long long)out_w ||
        (long long)tiles_y * GI2D_TILE < (long long)out_h)
        return fail("tile grid does not cover the picture");
    if (tiles_x > 0xffff || tiles_y > 0xffff || (long long)tiles_x * tiles_y * GI2D_FAST_LROW > 0x7fffffffLL ||
        (long long)tiles_x * tiles_y * num_pictures > 0x7fffffffLL)
        return fail("problem too large for 32-bit slot indices");
    const CodecBatchTable table = carve_codec_batch(batch, num_pictures);
    if (batch_bytes < table.bytes || ((uintptr_t)batch & 15)) return fail("batch table too small (gi2d_codec_batch_bytes) or misaligned");
    const int tiles = tiles_x * tiles_y;
    const size_t plane = pixel_plane_bytes(dtype, layout, out_h, out_w);
    std::vector<CodecBatchPicture> pics((size_t)num_pictures);
    CodecBatchAffines maps = {};
    bool any_affine = false;
    CodecBatchHead head = {};
    int max_n = 0;
    long long pg_total = 0;
    for (int k = 0; k < num_pictures; ++k) {
        const gi2d_codec_picture &d = pictures[k];
        const std::string who = "picture " + std::to_string(k);
        CodecBatchPicture &p = pics[(size_t)k];
        const int n = d.num_points;
        if (n < 0 || (long long)n * GI2D_FAST_S > 0x7fffffffLL) return fail(who + ": population negative or too large");
        if (const int rc = codec_stream_checked("codec decode batch: " + who, d.kind, n, d.xy_bits, d.p0_bits, d.p1_bits,
                                                d.color_bits, d.side, d.payload, d.payload_bytes, p.lay, p.side, p.last_dword))
            return rc;
        if (!d.status || !d.workspace) return fail(who + ": null or misaligned pointer");
        if (d.view == 2) {
            if (!affines) return fail(who + ": an affine view (view = 2) needs gi2d_codec_decode_batch_affine and its maps");
            const gi2d_codec_affine &a = affines[k];
            maps.af[k] = CodecAffine{a.x0, a.y0, a.b[0], a.b[1], a.b[2], a.b[3], a.prefilter[0], a.prefilter[1], a.prefilter[2]};
            if (const char *why = codec_affine_refused(maps.af[k], out_h, out_w, d.img_height, d.img_width))
                return fail(who + ": affine view: " + why);
            if (!std::isfinite(d.radius_clip)) return fail(who + ": affine view: radius_clip must be finite");
            any_affine = true;
        } else if (d.view) {
            if (const char *why = codec_view_refused(d.x0, d.y0, d.scale, out_h, out_w, d.img_height, d.img_width))
                return fail(who + ": view: " + why);
        } else if (d.img_height != out_h || d.img_width != out_w) {
            return fail(who + ": its size is not the call's and it has no view");
        }
        const FastWs w = carve_decode(d.workspace, n, tiles);
        if (d.workspace_bytes < w.bytes || ((uintptr_t)d.workspace & 15))
            return fail(who + ": workspace too small (gi2d_codec_decode_workspace_bytes) or misaligned");
        for (int j = 0; j < k; ++j) {  // a picture's workspace and status row are its own
            const char *a = (const char *)pictures[j].workspace, *b = (const char *)d.workspace;
            if ((a < b + w.bytes && b < a + pictures[j].workspace_bytes) || pictures[j].status == d.status)
                return fail(who + ": shares its workspace or status row with picture " + std::to_string(j));
        }
        p.payload = (const uint32_t *)d.payload;
        p.n = n;
        p.form = d.view == 2 ? 4 + (d.kind == kScaleRot ? 1 : 0) : (d.kind == kScaleRot ? 2 : 0) + (d.view ? 1 : 0);
        p.clip_coe = d.clip_coe;
        p.radius_clip = d.radius_clip;
        p.vw = d.view == 1 ? CodecView{d.x0, d.y0, d.scale} : CodecView{0.f, 0.f, 1.f};
        p.bt.colors = p.bt.opacities = nullptr;
        p.bt.prev_box = w.prev_box;
        p.bt.lists = w.lists;
        p.bt.recs = rec_sets(w, n);
        p.bt.status = d.status;
        p.tile_bins = (int2 *)w.tile_bins;
        p.out = (char *)out + (size_t)k * plane;
        head.pg_start[k] = (int)pg_total;
        head.tile_start[k] = k * tiles;
        pg_total += n > 0 ? (n + 255) / 256 : 1;  // (an empty picture still resets its status words)
        max_n = n > max_n ? n : max_n;
    }
    if (pg_total > 0x7fffffffLL) return fail("problem too large for 32-bit slot indices");
    head.pg_start[num_pictures] = (int)pg_total;
    head.tile_start[num_pictures] = num_pictures * tiles;
    // ---- the table, stream-ordered
    const hipStream_t s = (hipStream_t)st;
    CodecBatchPack pack;
    for (int k0 = 0; k0 < num_pictures; k0 += GI2D_CODEC_BATCH_PACK) {
        const int cnt = num_pictures - k0 < GI2D_CODEC_BATCH_PACK ? num_pictures - k0 : GI2D_CODEC_BATCH_PACK;
        for (int i = 0; i < cnt; ++i) pack.pic[i] = pics[(size_t)(k0 + i)];
        hipLaunchKernelGGL(codec_batch_write_kernel<CodecBatchPack>, dim3(1), dim3(256), 0, s, pack,
                           cnt * (int)(sizeof(CodecBatchPicture) / sizeof(int)), (int *)(table.pic + k0));
    }
    hipLaunchKernelGGL(codec_batch_write_kernel<CodecBatchHead>, dim3(1), dim3(256), 0, s, head,
                       (int)(sizeof(CodecBatchHead) / sizeof(int)), (int *)table.head);
    if (any_affine)
        hipLaunchKernelGGL(codec_batch_write_kernel<CodecBatchAffines>, dim3(1), dim3(256), 0, s, maps,
                           num_pictures * (int)(sizeof(CodecAffine) / sizeof(int)), (int *)table.affine);
    // ---- the three launches
    const int work = tiles > max_n ? tiles : max_n;
    const int reset_blocks = (work + 255) / 256;
    hipLaunchKernelGGL(codec_reset_batched_kernel, dim3((unsigned)(reset_blocks * num_pictures)), dim3(256), 0, s,
                       (const CodecBatchPicture *)table.pic, reset_blocks, tiles);
    const auto decode = any_affine ? codec_decode_bin_batched_kernel<true> : codec_decode_bin_batched_kernel<false>;
    hipLaunchKernelGGL(decode, dim3((unsigned)pg_total), dim3(256), 0, s, (const CodecBatchHead *)table.head,
                       (const CodecBatchPicture *)table.pic, (const CodecAffine *)table.affine, num_pictures, (float)out_w,
                       (float)out_h, tiles_x, tiles_y);
#define GI2D_DRAW_BATCH(D, L)                                                                                             \
    hipLaunchKernelGGL((any_affine ? codec_draw_batched_kernel<true, D, L> : codec_draw_batched_kernel<false, D, L>),     \
                       dim3((unsigned)(num_pictures * tiles)), dim3(256), 0, s, (const CodecBatchHead *)table.head,       \
                       (const CodecBatchPicture *)table.pic, num_pictures, tiles_x, tiles_y, (int)out_w, (int)out_h,      \
                       background)
    GI2D_FOR_FORMAT(dtype, layout, GI2D_DRAW_BATCH)
#undef GI2D_DRAW_BATCH
    return check_launch("codec decode batch");
}

}  // extern "C"
