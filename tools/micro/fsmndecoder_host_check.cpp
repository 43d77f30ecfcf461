// Stand-alone host check of the pf_fsmndecoder_* argument checks (csrc/engine_conformer.hip): every refusal of create() with the
// field its message must name, the null-argument refusals of the other entry points, and a create / destroy cycle. Needs no GPU:
// the limits are checked before any device call, and without a device an accepted config ends at the device check. Meant to be
// linked against the library's objects built with the host sanitizers, e.g. from funasr_amd/csrc:
//   S="-Xarch_host -fsanitize=address,undefined"; mkdir -p asan
//   for f in $(ls *.hip | grep -v gemm_f16x2_ffn); do hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -fPIC $S -c $f -o asan/${f%.hip}.o; done
//   hipcc -O1 -g -std=c++17 $S -c ../../tools/micro/fsmndecoder_host_check.cpp -o asan/check_main.o
//   hipcc --offload-arch=gfx950 -fsanitize=address,undefined asan/*.o -ldl -o asan/check && ./asan/check
// (gemm_f16x2_ffn.hip belongs to the measurement library only; asan/ is a scratch directory, nothing of it is kept)
#include <cstdio>
#include <cstring>

#include "../../include/paraformer_hip.h"

static int failures = 0;

static void expect(bool ok, const char* what) {
    if (!ok) { std::printf("FAILED: %s (last error: %s)\n", what, pf_last_error()); ++failures; }
}

int main() {
    const pf_fsmndecoder_config ok = {8404, 512, 4, 2048, 16, 16, 11, 0, 1e-12f};
    struct Case { const char* field; pf_fsmndecoder_config c; };
    Case cases[] = {
        {"vocab_size", ok}, {"n_heads", ok}, {"n_heads", ok}, {"d_model", ok}, {"ffn_dim", ok}, {"ffn_dim", ok}, {"kernel_size", ok},
        {"kernel_size", ok}, {"sanm_shift", ok}, {"sanm_shift", ok}, {"att_layer_num", ok}, {"att_layer_num", ok}, {"att_layer_num", ok},
        {"ln_eps", ok},
    };
    cases[0].c.vocab_size = 0;
    cases[1].c.n_heads = 0;
    cases[2].c.n_heads = 2;                                    // head dim 256
    cases[3].c.d_model = 4096; cases[3].c.n_heads = 32;
    cases[4].c.ffn_dim = 2040;
    cases[5].c.ffn_dim = 4096;
    cases[6].c.kernel_size = 0;
    cases[7].c.kernel_size = 33;
    cases[8].c.sanm_shift = 6;                                 // right padding 10 - 5 - 6 < 0
    cases[9].c.sanm_shift = -1;
    cases[10].c.att_layer_num = 0;
    cases[11].c.att_layer_num = 17;
    cases[12].c.n_blocks = 0;
    cases[13].c.ln_eps = 0.f;
    for (const Case& k : cases) {
        pf_fsmndecoder* h = pf_fsmndecoder_create(&k.c);
        expect(h == nullptr && std::strstr(pf_last_error(), k.field) != nullptr, k.field);
        pf_fsmndecoder_destroy(h);
    }
    expect(pf_fsmndecoder_create(nullptr) == nullptr && std::strstr(pf_last_error(), "null config") != nullptr, "null config");
    pf_fsmndecoder_destroy(nullptr);
    int32_t ids[2] = {1, 2};
    float x[4] = {0.f, 0.f, 0.f, 0.f};
    expect(pf_fsmndecoder_set_tensor(nullptr, "embed.0.weight", x, 4) == -1, "set_tensor(null handle)");
    expect(pf_fsmndecoder_missing(nullptr) == -1, "missing(null handle)");
    expect(pf_fsmndecoder_begin(nullptr, x, 1, 1, 1, nullptr) == -1, "begin(null handle)");
    expect(pf_fsmndecoder_step(nullptr, ids, 0, 2, x, nullptr) == -1, "step(null handle)");
    expect(pf_fsmndecoder_reorder(nullptr, ids, 2, nullptr) == -1, "reorder(null handle)");
    // an accepted config: a handle where a device is visible (layer table built, every tensor missing), else the device refusal
    pf_fsmndecoder* h = pf_fsmndecoder_create(&ok);
    if (h) {
        const int n_ffn3 = 2 + 2 + 2 + 1, n_att = n_ffn3 + 2 + 1 + 2 + 3 * 2;      // tensors of `decoders3`, of one `decoders` layer
        expect(pf_fsmndecoder_missing(h) == 1 + 16 * n_att + n_ffn3 + 2 + 2, "tensor count of the layer table");
        expect(pf_fsmndecoder_set_tensor(h, "decoders.16.norm1.weight", x, 4) == -1, "unknown tensor name");
        expect(pf_fsmndecoder_begin(h, x, 1, 1, 257, nullptr) == -1 && std::strstr(pf_last_error(), "max_hyp") != nullptr, "max_hyp");
        expect(pf_fsmndecoder_begin(h, x, 1, 5001, 1, nullptr) == -1 && std::strstr(pf_last_error(), "max_len") != nullptr, "max_len");
        expect(pf_fsmndecoder_step(h, ids, 0, 2, x, nullptr) == -1, "step before begin");
        pf_fsmndecoder_destroy(h);
        std::printf("device visible: create / refuse / destroy on a real handle\n");
    } else {
        std::printf("no device: the accepted config ends at the device check (%s)\n", pf_last_error());
    }
    std::printf(failures ? "%d check(s) FAILED\n" : "all checks passed\n", failures);
    return failures ? 1 : 0;
}
