// The loss launches of gi2d_train_steps_loss / gi2d_train_steps_loss_batched (gi2d_loss.hip), as gi2d_train.hip's driver
// calls them.
#pragma once
#include "gi2d_common.h"

namespace gi2d {

// Weights (w2, w1, ws) of a loss type's terms -- mean d^2, mean |d|, 1 - structural value -- and the structural term's
// form: levels 0 (none), 1 (SSIM) or 5 (MS-SSIM) with window `win`.  Doubles, like the Python floats of
// models/utils.py:60-80.  False: unknown type or lambda outside [0, 1].
struct LossTerms {
    double w2, w1, ws;
    int levels, win;
};
bool loss_terms(int type, double lambda, LossTerms &t);

// The regions of a gi2d_train_loss::workspace.
struct LossWs {
    float *x;       // [H, W, 3] clamp(out_img, 0, 1): what the SSIM entries read (structural types only)
    float *v;       // [H, W, 3] v_output of gi2d_train_steps_loss
    float *result;  // [GI2D_SSIM_RESULT_FLOATS] of the SSIM forward, then grad_result[3] at [64], one pad word
    float *tile_abs;  // [tiles] per-tile sum of |d|
    void *ssim;
    size_t ssim_bytes, bytes;
};
// bytes == 0: the type cannot take this size (the message is set)
LossWs carve_loss(void *base, int h, int w, const LossTerms &t);

// The constants of the per-pixel terms: they depend on the image's size through P = 3 H W.
struct LossPixel {
    float c2, c1;  // 2 w2 / P, w1 / P
    float gres;    // -ws / 3: the upstream gradient of every channel's structural value
};
// ... and of the scalar loss: w2 / P, w1 / P (ws is the same for every image of a call)
struct LossScalar {
    float w2_over_p, w1_over_p;
};
LossPixel loss_pixel(int h, int w, const LossTerms &t);
LossScalar loss_scalar(int h, int w, const LossTerms &t);

// out_img, gt -> v (the gradient image), tile_sse, loss_value; only enqueues.
int loss_launch(const float *out_img, const float *gt, int h, int w, const LossTerms &t, const LossWs &ws, float *v,
                float *tile_sse, float *loss_value, hipStream_t st);

// What a batch of loss launches owns beside its images' own workspaces (gi2d_train_loss_batch_workspace_bytes): the
// contiguous results and upstream gradients the batched SSIM entries ask for, and their batch workspace.
struct LossBatchWs {
    float *results;       // [K][GI2D_SSIM_RESULT_FLOATS]
    float *grad_results;  // [K][3]
    void *ssim;
    size_t ssim_bytes, bytes;
};
// heights / widths: K host ints.  bytes == 0: a size the type cannot take (the message is set)
LossBatchWs carve_loss_batch(void *base, int k, const int *heights, const int *widths, const LossTerms &t);

}  // namespace gi2d
