// Host-side sanitizer check of the batched rANS expansion's argument checks (gi2d_codec_rans_expand_batch): a stand-alone
// program that feeds the entry the refused argument sets of tests/test_codec_rans_batch_cpu.py.  Every call is refused
// before any device call, so this runs on a machine without a GPU.  Build it with the host side of the library's sources
// under AddressSanitizer and UBSan, from the repository root:
//     hipcc -O1 -g -std=c++17 --offload-arch=gfx950 -Xarch_host -fsanitize=address,undefined -Iinclude \
//         -Igaussianimage_plus_amd/csrc tools/rans_batch_refusals.cpp gaussianimage_plus_amd/csrc/gi2d_rans.hip \
//         gaussianimage_plus_amd/csrc/gi2d_capi.hip -o build/rans_batch_refusals && build/rans_batch_refusals
#include <cstdio>
#include <cstring>
#include <vector>

#include "gi2d.h"

static int failures = 0;
static void expect(int rc, const char *word, const char *what) {
    const char *msg = gi2d_last_error_string();
    if (rc != GI2D_ERR_INVALID_ARGUMENT || !msg || !strstr(msg, word)) {
        std::printf("FAILED %s: rc %d, message '%s' (expected '%s')\n", what, rc, msg ? msg : "", word);
        ++failures;
    }
}

static gi2d_codec_rans_stream good_stream() {
    gi2d_codec_rans_stream d = {};
    void *p = (void *)(uintptr_t)64;  // never dereferenced
    d.kind = 1, d.num_points = 3000, d.xy_bits = 12, d.p0_bits = 10, d.p1_bits = 0, d.color_bits = 6, d.chunk_log2 = 10;
    d.coded_mask = 0xFC, d.delta_mask = 0;
    d.tables = p, d.tables_bytes = 6 * 4612;
    d.directory = p, d.chunk_data = p, d.chunk_data_bytes = 3 * 8000, d.max_chunk_bytes = 8000;
    d.payload = p, d.payload_bytes = 4 * ((3000 * 72 + 31) / 32), d.status = (int32_t *)p;
    return d;
}

int main() {
    size_t last = 0;
    for (int k = 1; k <= 64; ++k) {
        const size_t b = gi2d_codec_rans_batch_bytes(k);
        if (b <= last) std::printf("FAILED batch bytes do not grow at %d\n", k), ++failures;
        last = b;
    }
    std::vector<gi2d_codec_rans_stream> s(65, good_stream());
    void *table = (void *)(uintptr_t)256;
    const size_t big = (size_t)1 << 40;
    expect(gi2d_codec_rans_expand_batch(0, s.data(), table, big, 1, nullptr), "1 .. 64", "0 streams");
    expect(gi2d_codec_rans_expand_batch(65, s.data(), table, big, 1, nullptr), "1 .. 64", "65 streams");
    expect(gi2d_codec_rans_expand_batch(3, s.data(), nullptr, big, 1, nullptr), "null", "null table");
    expect(gi2d_codec_rans_expand_batch(3, s.data(), (void *)(uintptr_t)264, big, 1, nullptr), "misaligned", "misaligned table");
    expect(gi2d_codec_rans_expand_batch(3, s.data(), table, 64, 1, nullptr), "too small", "small table");
    expect(gi2d_codec_rans_expand_batch(64, s.data(), table, last - 1, 1, nullptr), "too small", "table one byte short");
    expect(gi2d_codec_rans_expand_batch(3, nullptr, table, big, 1, nullptr), "null", "null entries");
    s[1].delta_mask = 1;
    expect(gi2d_codec_rans_expand_batch(64, s.data(), table, big, 1, nullptr), "stream 1:", "delta mask outside coded mask");
    s[1] = good_stream(), s[2].payload_bytes -= 4;
    expect(gi2d_codec_rans_expand_batch(64, s.data(), table, big, 1, nullptr), "stream 2:", "short output");
    s[2] = good_stream(), s[63].max_chunk_bytes = 8001;
    expect(gi2d_codec_rans_expand_batch(64, s.data(), table, big, 1, nullptr), "stream 63:", "odd max_chunk_bytes");
    s[63] = good_stream(), s[0].status = nullptr;
    expect(gi2d_codec_rans_expand_batch(64, s.data(), table, big, 1, nullptr), "stream 0:", "null status");
    std::printf(failures ? "%d checks failed\n" : "all refusals as expected (%d failures)\n", failures);
    return failures ? 1 : 0;
}
