// Host-side sanitizer check of the fitting entries' argument checks (gi2d_train_steps, gi2d_train_step,
// gi2d_train_steps_loss, gi2d_train_steps_batched, gi2d_train_steps_loss_batched): a stand-alone program that calls them
// with argument sets every one of which is refused, or returns idle, before any device call, so it runs on a machine
// without a GPU.  The cases are those of test_what_the_single_image_entries_test_first (tests/test_call_outputs_gpu.py),
// test_batched_entry_rejects_bad_batches (tests/test_batched_gpu.py), test_entry_refuses_mixed_batches_and_unfit_sizes
// (tests/test_loss_batch_gpu.py) and the refusals of quant_of and loss_check (gi2d_train.hip), with the pairs that show
// which of two refusals an entry reports first.  One line per case: entry, return code, gi2d_last_error_string() ("-" for
// a call that returned GI2D_OK).  The C ABI being what it is, the output of this program linked against an earlier
// revision of the library is the expectation for a later one: keep both and compare them.  Build it with the host side of
// the library's sources under AddressSanitizer and UBSan, from the repository root:
//     hipcc -O1 -g -std=c++17 --offload-arch=gfx950 -Xarch_host -fsanitize=address,undefined -Iinclude \
//         -Igaussianimage_plus_amd/csrc tools/fit_refusals.cpp gaussianimage_plus_amd/csrc/*.hip \
//         -o build/fit_refusals && build/fit_refusals
#include <cstdint>
#include <cstdio>
#include <vector>

#include "gi2d.h"

// Pointers are fake addresses, 4 KB apart and never dereferenced.
static uintptr_t next_address = (uintptr_t)1 << 32;
template <class T>
static T *fake() {
    next_address += 4096;
    return (T *)next_address;
}

static const int H = 32, W = 48, N = 64, TX = 3, TY = 2;  // the shape of the single-image test
static const double LR[3] = {1e-3, 1e-3, 1e-3};

static gi2d_train_state good_state(int kind = 0) {
    gi2d_train_state s = {};
    s.kind = kind, s.num_points = N, s.img_height = H, s.img_width = W;
    s.clip_coe = 3.f, s.radius_clip = 1.f;
    s.xyz = fake<float>(), s.chol = fake<float>(), s.feat = fake<float>();
    s.opacity = fake<float>(), s.bound = fake<float>();
    s.m_xyz = fake<float>(), s.v_xyz = fake<float>(), s.m_chol = fake<float>(), s.v_chol = fake<float>();
    s.m_feat = fake<float>(), s.v_feat = fake<float>();
    s.gt = fake<float>(), s.xys = fake<float>(), s.conics = fake<float>();
    s.radii = fake<int32_t>(), s.num_tiles_hit = fake<int32_t>();
    s.out_img = fake<float>(), s.tile_sse = fake<float>(), s.status = fake<int32_t>();
    s.workspace = fake<void>(), s.workspace_bytes = gi2d_fast_workspace_bytes(N, TX, TY);
    s.beta3 = 0.99;
    return s;
}

static gi2d_train_quant good_quant() {
    gi2d_train_quant q = {};
    q.xy_bits = 12, q.cov_bits = 10, q.color_bits = 6, q.rot_bits = 8, q.defer_capacity = 64;
    q.qparams = fake<float>(), q.qm = fake<float>(), q.qv = fake<float>(), q.range = fake<float>();
    q.qfeat = fake<float>(), q.partial = fake<float>(), q.defer = fake<int32_t>();
    for (int c = 0; c < 3; ++c) q.lr[c] = 1e-4, q.eps[c] = 1e-8f;
    q.beta1 = 0.9, q.beta2 = 0.999, q.first_step = 1;
    return q;
}

static gi2d_train_loss good_loss(int type = 4) {
    gi2d_train_loss l = {};
    l.type = type, l.lambda = 0.7f;
    l.workspace = fake<void>(), l.workspace_bytes = gi2d_train_loss_workspace_bytes(H, W, type);
    l.loss_value = fake<float>();
    return l;
}

static void line(const char *entry, const char *what, int rc) {
    const char *msg = gi2d_last_error_string();
    std::printf("%-30s %-52s %3d  %s\n", entry, what, rc, rc == GI2D_OK ? "-" : (msg ? msg : "(null)"));
}

// gi2d_train_steps and gi2d_train_steps_loss open alike: both get every case that does not concern the loss
static void both(const char *what, const gi2d_train_state *s, const double *lr, int first_step, int count) {
    const gi2d_train_loss loss = good_loss();
    line("gi2d_train_steps", what, gi2d_train_steps(s, lr, 0.9, 0.999, 1e-8f, first_step, count, nullptr));
    line("gi2d_train_steps_loss", what, gi2d_train_steps_loss(s, &loss, lr, 0.9, 0.999, 1e-8f, first_step, count, nullptr));
}
static void lossy(const char *what, const gi2d_train_state *s, const gi2d_train_loss *loss) {
    line("gi2d_train_steps_loss", what, gi2d_train_steps_loss(s, loss, LR, 0.9, 0.999, 1e-8f, 1, 3, nullptr));
}

static void single_image_cases() {
    const gi2d_train_state good = good_state();
    gi2d_train_state s = good;
    both("null lr", &good, nullptr, 1, 3);
    both("first step 0", &good, LR, 0, 3);
    both("count 0: idle", &good, LR, 1, 0);
    both("count 0, null lr, first step 0: idle", &good, nullptr, 0, 0);
    s.xyz = nullptr;
    both("count 0, null xyz: an idle call checks the state", &s, LR, 1, 0);
    s = good, s.num_points = 0;
    both("no gaussians: idle", &s, LR, 1, 3);
    both("no gaussians, null lr: idle", &s, nullptr, 0, 3);
    line("gi2d_train_step", "step 0", gi2d_train_step(&good, LR, 0.9, 0.999, 1e-8f, 0, nullptr));
    line("gi2d_train_step", "null lr", gi2d_train_step(&good, nullptr, 0.9, 0.999, 1e-8f, 1, nullptr));
    // every test on the state
    both("null state", nullptr, LR, 1, 3);
    s = good, s.kind = 3;
    both("kind 3", &s, LR, 1, 3);
    s = good, s.img_width = 0;
    both("width 0", &s, LR, 1, 3);
    s = good, s.status = nullptr;
    both("null status", &s, LR, 1, 3);
    s = good, s.workspace_bytes -= 1;
    both("workspace one byte short", &s, LR, 1, 3);
    s = good, s.workspace = nullptr;
    both("null workspace", &s, LR, 1, 3);
    s = good, s.optimizer = 2;
    both("optimizer 2", &s, LR, 1, 3);
    both("optimizer 2 and null lr: the state first", &s, nullptr, 1, 3);
    both("optimizer 2, count 0: idle", &s, LR, 1, 0);
    s = good, s.optimizer = 1;
    both("Adan without d_* / pg_*", &s, LR, 1, 3);
    s = good, s.best_sse = fake<float>();
    both("best_sse without the snapshot buffers", &s, LR, 1, 3);
    // the quantisers
    gi2d_train_quant q = good_quant();
    s = good, s.quant = &q;
    both("quantised cholesky model", &s, LR, 1, 3);
    s = good_state(1), s.quant = &q, s.optimizer = 1;
    s.d_xyz = s.d_chol = s.d_feat = s.pg_xyz = s.pg_chol = s.pg_feat = fake<float>();
    both("quantised fit with Adan", &s, LR, 1, 3);
    s = good_state(1), s.quant = &q;
    q.first_step = 0;
    both("quantiser step 0", &s, LR, 1, 3);
    q = good_quant(), q.xy_bits = 17;
    both("xy_bits 17", &s, LR, 1, 3);
    q = good_quant(), q.color_bits = 0;
    both("color_bits 0", &s, LR, 1, 3);
    q = good_quant(), q.qfeat = nullptr;
    both("null qfeat", &s, LR, 1, 3);
    q = good_quant(), q.range = nullptr;
    both("covariance model without range", &s, LR, 1, 3);
    q = good_quant(), q.defer_capacity = 1;
    both("covariance model, defer_capacity 1", &s, LR, 1, 3);
    q = good_quant(), q.xy_bits = 0;
    both("xy_bits 0 and null lr: lr first", &s, nullptr, 1, 3);
    gi2d_train_state rs = good_state(2);
    rs.quant = &q;
    q = good_quant(), q.rot_bits = 1;
    both("rotation-scale model, rot_bits 1", &rs, LR, 1, 3);
    q = good_quant(), q.qparams = (float *)((uintptr_t)q.qparams + 4);
    both("rotation-scale model, qparams misaligned", &rs, LR, 1, 3);
    // the loss
    gi2d_train_loss l = good_loss();
    lossy("null loss", &good, nullptr);
    l.type = 8;
    lossy("loss type 8", &good, &l);
    l = good_loss(), l.lambda = 1.5f;
    lossy("lambda 1.5", &good, &l);
    l = good_loss(), l.type = 6;
    lossy("Fusion4 at 32x48", &good, &l);
    l = good_loss(), l.loss_value = nullptr;
    lossy("null loss_value", &good, &l);
    l = good_loss(), l.workspace = nullptr;
    lossy("null loss workspace", &good, &l);
    l = good_loss(), l.workspace = (char *)l.workspace + 16;
    lossy("loss workspace misaligned", &good, &l);
    l = good_loss(), l.workspace_bytes -= 1;
    lossy("loss workspace one byte short", &good, &l);
    l = good_loss(), l.type = 8;
    s = good_state(1), s.quant = &q, q = good_quant(), q.xy_bits = 0;
    lossy("loss type 8 and xy_bits 0", &s, &l);
    s = good, s.optimizer = 2;
    lossy("loss type 8 and optimizer 2", &s, &l);
    line("gi2d_train_steps_loss", "loss type 8, count 0: idle",
         gi2d_train_steps_loss(&good, &l, LR, 0.9, 0.999, 1e-8f, 1, 0, nullptr));
}

struct Batch {
    std::vector<const gi2d_train_state *> states;
    std::vector<const gi2d_train_loss *> losses;
    void *table = fake<void>(), *loss_ws = fake<void>();
    size_t table_bytes = 0, loss_ws_bytes = 0;
    const double *lr = LR;
    int first_step = 1, count = 1;
    Batch(std::vector<const gi2d_train_state *> s, std::vector<const gi2d_train_loss *> l) : states(s), losses(l) {
        const std::vector<int> hs(s.size(), H), ws(s.size(), W);
        table_bytes = gi2d_batch_bytes((int)s.size());
        loss_ws_bytes = gi2d_train_loss_batch_workspace_bytes((int)s.size(), hs.data(), ws.data(), 4);
    }
    void plain(const char *what, int k = -1) const {
        line("gi2d_train_steps_batched", what,
             gi2d_train_steps_batched(k < 0 ? (int)states.size() : k, states.data(), table, table_bytes, lr, 0.9, 0.999,
                                      1e-8f, first_step, count, nullptr));
    }
    void lossy(const char *what, int k = -1) const {
        line("gi2d_train_steps_loss_batched", what,
             gi2d_train_steps_loss_batched(k < 0 ? (int)states.size() : k, states.data(), losses.data(), table,
                                           table_bytes, loss_ws, loss_ws_bytes, lr, 0.9, 0.999, 1e-8f, first_step,
                                           count, nullptr));
    }
    void both(const char *what, int k = -1) const { plain(what, k), lossy(what, k); }
};

static void batched_cases() {
    const gi2d_train_state a = good_state(0), c = good_state(0), cov = good_state(1);
    const gi2d_train_loss la = good_loss(), lc = good_loss();
    gi2d_train_state s = a;
    const Batch good({&a, &c}, {&la, &lc});
    Batch b = good;
    // the call's own arguments
    b.both("0 images", 0);
    b.both("65 images", 65);
    line("gi2d_train_steps_batched", "null states",
         gi2d_train_steps_batched(2, nullptr, b.table, b.table_bytes, LR, 0.9, 0.999, 1e-8f, 1, 1, nullptr));
    line("gi2d_train_steps_loss_batched", "null losses",
         gi2d_train_steps_loss_batched(2, b.states.data(), nullptr, b.table, b.table_bytes, b.loss_ws, b.loss_ws_bytes, LR,
                                       0.9, 0.999, 1e-8f, 1, 1, nullptr));
    b.table_bytes = 64;
    b.both("table of 64 bytes");
    b = good, b.table = nullptr;
    b.both("null table");
    b = good, b.table = (char *)b.table + 4;
    b.both("table not 16-byte aligned");
    b = good, b.loss_ws = nullptr;
    b.lossy("null batch loss workspace");
    b = good, b.loss_ws = (char *)b.loss_ws + 16;
    b.lossy("batch loss workspace misaligned");
    b = good, b.count = 0, b.states[1] = nullptr;
    b.both("count 0 with a null state: idle before any state");
    b.table_bytes = 64;
    b.both("count 0 and a table of 64 bytes: the table first");
    b = good, b.lr = nullptr;
    b.both("null lr");
    b = good, b.first_step = 0;
    b.both("first step 0");
    b.states[0] = nullptr;
    b.both("first step 0 and a null state: the step first");
    // every test on one state
    b = good, b.states[1] = nullptr;
    b.both("image 1: null state");
    s.gt = nullptr, b.states[1] = &s;
    b.both("image 1: null gt");
    s = a, s.workspace_bytes -= 1;
    b.both("image 1: workspace one byte short");
    s = a, s.optimizer = 2;
    b.both("image 1: optimizer 2");
    s = a, s.optimizer = 1;
    b.both("image 1: Adan without d_* / pg_*");
    s = a, s.best_sse = fake<float>();
    b.both("image 1: best_sse without the snapshot buffers");
    b.states = {&s, &c};
    b.both("image 0: best_sse without the snapshot buffers");
    // what the images of a batch share
    b = good, b.states[1] = &cov;
    b.both("cholesky and covariance model");
    s = a, s.beta3 = 0.9;
    b.states[1] = &s;
    b.both("beta3 differs");
    gi2d_train_quant q0 = good_quant(), q1 = good_quant();
    gi2d_train_state c0 = good_state(1), c1 = good_state(1);
    c1.quant = &q1;
    b.states = {&c0, &c1};
    b.both("one image of two quantised");
    c0.quant = &q0, q1.cov_bits = 11;
    b.both("quantisers of different bit depths");
    q1 = good_quant(), q1.eps[2] = 1e-6f;
    b.both("quantisers of different eps");
    q1 = good_quant(), q1.first_step = 0;
    b.both("image 1: quantiser step 0");
    q1 = good_quant(), q1.range = nullptr;
    b.both("image 1: covariance model without range");
    q0.xy_bits = q1.xy_bits = 0, q1.range = fake<float>();
    b.both("xy_bits 0 in both");
    c0.kind = c1.kind = 0, q0 = q1 = good_quant();
    b.both("quantised cholesky models");
    // the loss
    gi2d_train_loss l = la;
    b = good, b.losses[1] = nullptr;
    b.lossy("image 1: null loss");
    b.losses[1] = &l, l.type = 1, l.workspace_bytes = gi2d_train_loss_workspace_bytes(H, W, 1);
    b.lossy("loss types 4 and 1");
    l = la, l.lambda = 0.5f;
    b.lossy("lambda 0.7 and 0.5");
    l = la, l.type = 6;
    b.losses = {&l, &l};
    b.lossy("Fusion4 at 32x48");
    l = la, l.type = 8;
    b.lossy("loss type 8");
    l = la, l.loss_value = nullptr;
    b.losses = {&la, &l};
    b.lossy("image 1: null loss_value");
    l = la, l.workspace_bytes -= 1;
    b.lossy("image 1: loss workspace one byte short");
    l = la, l.workspace = (char *)l.workspace + 16;
    b.lossy("image 1: loss workspace misaligned");
    b = good, b.loss_ws_bytes -= 1;
    b.lossy("batch loss workspace one byte short");
    // which of two refusals comes first
    l = la, l.type = 8;
    b = good, b.losses[1] = &l, b.states[1] = &cov;
    b.lossy("two model kinds and image 1: loss type 8");
    c0 = c1 = good_state(1), c0.quant = &q0, c1.quant = &q1, q0 = q1 = good_quant(), q0.xy_bits = q1.xy_bits = 0;
    b.states = {&c0, &c1}, b.losses = {&l, &l};
    b.lossy("xy_bits 0 and loss type 8 in both");
    b.losses = {&l, &la}, q0 = q1 = good_quant(), q1.xy_bits = 0;
    b.lossy("image 0: loss type 8, image 1: xy_bits 0");
}

int main() {
    single_image_cases();
    batched_cases();
    return 0;
}
