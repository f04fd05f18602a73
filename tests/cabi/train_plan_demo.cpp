// csrc/vs_train_plan.h alone, as plain C++17 (no HIP): tests/test_train_plan_host.py builds this with the host compiler and
// -fsanitize=address,undefined.  Part 1: named cases -> the expected plan (every attention enumerator and every mode-word value
// the grid can produce is reached); part 2: what each switch flips; part 3: invariants over a grid;
// part 4: every handed-back form word against the validation rule; part 5: the argument refusals and their precedence.
// Prints "OK" or the first failed check.
#include <cstdio>
#include <cstring>
#include <set>
#include <string>
#include <utility>

#include "vs_train_plan.h"

#define CHECK(...) do { if (!(__VA_ARGS__)) { std::printf("FAILED line %d: %s\n", __LINE__, #__VA_ARGS__); return 1; } } while (0)

namespace {

const unsigned LIN = VS_TRAIN_FLAG_BF16_LINEAR, ATT = VS_TRAIN_FLAG_BF16_ATTENTION, BF16 = VS_TRAIN_FLAG_BF16, FP16 = VS_TRAIN_FLAG_FP16,
               OPT_IN = VS_TRAIN_FLAG_PACKED_LP_ATTENTION;
const int S = VSK_STORE16, A = VSK_A16, F = VSK_F16, Y = VST_WGRAD_Y16, X = VST_WGRAD_X16;

VskOptions defaults() {
    VskOptions o{};
    o.skinny_rows = 16384; o.lp_min_rows = 8192; o.lp_min_rows_fused = 256; o.train_lp_min_rows = 1024; o.attn_w64 = 1;
    return o;
}
VskOptions with(int VskOptions::*field, int value) { VskOptions o = defaults(); o.*field = value; return o; }

// a model with a positional table of 20000 rows; a padded or packed forward or backward on it
VsTrainIn call(int d, int heads, int B, int T, unsigned flags, bool packed = false, bool backward = false, unsigned reserved = 0, float p = 0.f) {
    return VsTrainIn{d, heads, 20000, true, packed ? 1 : B, packed ? B * T : T, packed, flags, p, 0.f, reserved, backward};
}
VsTrainIn backward(VsTrainIn in, unsigned reserved = 0) { in.backward = true; in.reserved = reserved; return in; }

enum Field { F_LP, F_LPA, F_QKV16, F_H16, F_ROWS16, F_F16, F_FORMAT, F_ATTENTION, F_KV_STRIDE, F_QKV_ROWS16, F_FAMILIES, F_T_FRAGMENTS, F_T16,
             F_LINEAR, F_QKV, F_FC1, F_FC2, F_ATT, F_OUT16, F_ROWDOT, F_WGRAD_W2, F_GATE, F_WGRAD_W1, F_DGRAD_FC1, F_DATT, F_WGRAD_QKV, F_DGRAD_QKV,
             F_COUNT };
unsigned bit(Field f) { return 1u << f; }
const unsigned FORM_STORAGE = bit(F_QKV16) | bit(F_H16), MODES_QKV = bit(F_QKV) | bit(F_ATT) | bit(F_OUT16) | bit(F_ROWDOT) | bit(F_DATT) | bit(F_WGRAD_QKV) | bit(F_DGRAD_QKV),
               MODES_HIDDEN = bit(F_FC1) | bit(F_FC2) | bit(F_WGRAD_W2) | bit(F_GATE) | bit(F_WGRAD_W1) | bit(F_DGRAD_FC1);
void values(const VsTrainPlan &p, long long v[F_COUNT]) {
    const long long a[F_COUNT] = {p.form.lp, p.form.lpa, p.form.qkv16, p.form.h16, p.form.rows16, p.form.f16, p.format, p.attention, (long long)p.kv_stride,
                                  p.qkv_rows16, p.families, p.transposed_fragments, p.t16, p.mode_linear, p.mode_qkv, p.mode_fc1, p.mode_fc2,
                                  p.mode_attention, p.attention_out16, p.mode_rowdot, p.mode_wgrad_w2, p.mode_gate, p.mode_wgrad_w1, p.mode_dgrad_fc1,
                                  p.mode_datt, p.mode_wgrad_qkv, p.mode_dgrad_qkv};
    std::memcpy(v, a, sizeof a);
}
// the fields in which two plans differ
unsigned differing(const VsTrainPlan &a, const VsTrainPlan &b) {
    long long va[F_COUNT], vb[F_COUNT];
    values(a, va); values(b, vb);
    unsigned m = 0;
    for (int f = 0; f < F_COUNT; ++f) if (va[f] != vb[f]) m |= 1u << f;
    return m;
}

// ---- part 1: the table.  A Want is everything of the plan that does not depend on the batch's size or the direction ----
struct Want {
    VsTrainForm form; uint32_t format; bool kv_half;
    int mode_linear, mode_qkv, mode_fc1, mode_fc2, mode_attention; bool attention_out16;
    int mode_rowdot, mode_wgrad_w2, mode_gate, mode_wgrad_w1, mode_dgrad_fc1, mode_datt, mode_wgrad_qkv, mode_dgrad_qkv;
};
//                          lp     lpa    qkv16  h16    rows16 f16      format      half   lin    qkv        fc1        fc2        att    out16  rowdot wgrad_w2   gate       wgrad_w1   dgrad_fc1  datt       wgrad_qkv  dgrad_qkv
const Want EXACT{         {false, false, false, false, false, false}, 0x80000000u, false, 0,     0,         0,         0,         0,     false, 0,     0,         0,         0,         0,         0,         0,         0};
const Want LINEAR16{      {true,  false, false, true,  false, false}, 0x80000009u, false, 1,     1,         1 | S,     1 | A,     0,     false, 0,     1 | X,     1 | S,     1 | Y,     1 | A,     1,         1,         1};
const Want ATTENTION16{   {false, true,  false, false, false, false}, 0x80000002u, false, 0,     0,         0,         0,         0,     false, 2,     0,         0,         0,         0,         0,         0,         0};
const Want BOTH16{        {true,  true,  true,  true,  false, false}, 0x8000000fu, true,  1,     1 | S,     1 | S,     1 | A,     1,     true,  1,     1 | X,     1 | S,     1 | Y,     1 | A,     1 | S,     1 | Y,     1 | A};
const Want BOTH16_ROWS{   {true,  true,  true,  true,  true,  false}, 0x8000001fu, true,  1,     1 | S,     1 | S,     1 | A,     1,     true,  1,     1 | X,     1 | S,     1 | Y,     1 | A,     1 | S,     1 | Y,     1 | A};
const Want LINEAR16_ROWS{ {true,  false, false, true,  true,  false}, 0x80000019u, false, 1,     1,         1 | S,     1 | A,     0,     false, 0,     1 | X,     1 | S,     1 | Y,     1 | A,     1,         1,         1};
const Want BOTH_STORE32{  {true,  true,  false, false, false, false}, 0x80000003u, false, 1,     1,         1,         1,         0,     false, 2,     1,         1,         1,         1,         1,         1,         1};
const Want PACKED_BOTH16{ {true,  true,  false, true,  false, false}, 0x8000000bu, false, 1,     1,         1 | S,     1 | A,     0,     false, 2,     1 | X,     1 | S,     1 | Y,     1 | A,     1,         1,         1};
const Want FP16_BOTH{     {true,  true,  true,  true,  false, true},  0x8000002fu, true,  1 | F, 1 | S | F, 1 | S | F, 1 | A | F, 1 | F, true,  1 | F, 1 | X | F, 1 | S | F, 1 | Y | F, 1 | A | F, 1 | S | F, 1 | Y | F, 1 | A | F};
const Want FP16_LINEAR{   {true,  false, false, true,  false, true},  0x80000029u, false, 1 | F, 1 | F,     1 | S | F, 1 | A | F, F,     false, 0,     1 | X | F, 1 | S | F, 1 | Y | F, 1 | A | F, 1 | F,     1 | F,     1 | F};
const Want FP16_ATTENTION{{false, true,  false, false, false, true},  0x80000022u, false, 0,     0,         0,         0,         F,     false, 2 | F, 0,         0,         0,         0,         0,         0,         0};
const Want FP16_PACKED{   {true,  true,  false, true,  false, true},  0x8000002bu, false, 1 | F, 1 | F,     1 | S | F, 1 | A | F, F,     false, 2 | F, 1 | X | F, 1 | S | F, 1 | Y | F, 1 | A | F, 1 | F,     1 | F,     1 | F};
const Want FP16_STORE32{  {true,  true,  false, false, false, true},  0x80000023u, false, 1 | F, 1 | F,     1 | F,     1 | F,     F,     false, 2 | F, 1 | F,     1 | F,     1 | F,     1 | F,     1 | F,     1 | F,     1 | F};

struct Case { const char *name; VsTrainIn in; VskOptions opt; Want want; VsTrainAttention attention; };

std::set<std::pair<int, long long>> g_seen;       // (field, value) reached by a named case

// the full expected plan of a case: the Want, and what follows from the batch's size and the direction
VsTrainPlan expected(const Case &c) {
    const Want &w = c.want;
    const size_t plane = (size_t)c.in.B * c.in.T * c.in.d_model;
    const bool skinny = c.in.B * c.in.T <= c.opt.skinny_rows;
    VsTrainPlan e{};
    e.form = w.form; e.format = w.format; e.attention = c.attention; e.kv_stride = w.kv_half ? plane / 2 : plane;
    e.qkv_rows16 = w.form.rows16 && w.form.qkv16;
    e.families = c.in.backward ? 0u : (skinny ? (unsigned)VSW_FRAGMENTS : 0u) | (w.form.rows16 ? (unsigned)VSW_ROWS16 : 0u);
    e.transposed_fragments = c.in.backward && skinny;
    e.t16 = c.in.backward && w.form.rows16;
    e.mode_linear = w.mode_linear; e.mode_qkv = w.mode_qkv; e.mode_fc1 = w.mode_fc1; e.mode_fc2 = w.mode_fc2; e.mode_attention = w.mode_attention;
    e.attention_out16 = w.attention_out16; e.mode_rowdot = w.mode_rowdot; e.mode_wgrad_w2 = w.mode_wgrad_w2; e.mode_gate = w.mode_gate;
    e.mode_wgrad_w1 = w.mode_wgrad_w1; e.mode_dgrad_fc1 = w.mode_dgrad_fc1; e.mode_datt = w.mode_datt; e.mode_wgrad_qkv = w.mode_wgrad_qkv;
    e.mode_dgrad_qkv = w.mode_dgrad_qkv;
    return e;
}

bool plan_is(const Case &c) {
    VsTrainPlan p;
    std::string err;
    if (vs_train_plan(c.in, c.opt, &p, &err) != VS_OK) { std::printf("%s: refused: %s\n", c.name, err.c_str()); return false; }
    if (const unsigned m = differing(p, expected(c))) { std::printf("%s: plan differs from the table in fields 0x%x\n", c.name, m); return false; }
    long long v[F_COUNT];
    values(p, v);
    for (int f = F_ATTENTION; f < F_COUNT; ++f) if (f != F_KV_STRIDE) g_seen.insert({f, v[f]});
    return true;
}

const int R16 = 192 * 256;      // rows from which the A-stationary kernels engage by themselves
const Case kCases[] = {
    // d_model 256, 4 heads (head dim 64), padded
    {"exact", call(256, 4, 2, 1000, 0), defaults(), EXACT, VST_ATT_PADDED_EXACT},
    {"exact, backward", backward(call(256, 4, 2, 1000, 0)), defaults(), EXACT, VST_ATT_PADDED_EXACT},
    {"exact above skinny_rows: no image family", call(256, 4, 1, 16385, 0), defaults(), EXACT, VST_ATT_PADDED_EXACT},
    {"exact above skinny_rows, backward: no transposed fragments", backward(call(256, 4, 1, 16385, 0)), defaults(), EXACT, VST_ATT_PADDED_EXACT},
    {"bf16 at train_lp_min_rows: exact", call(256, 4, 1, 1024, BF16), defaults(), EXACT, VST_ATT_PADDED_EXACT},
    {"bf16 at train_lp_min_rows + 1", call(256, 4, 1, 1025, BF16), defaults(), BOTH16, VST_ATT_PADDED16},
    {"bf16 at train_lp_min_rows + 1, backward", backward(call(256, 4, 1, 1025, BF16)), defaults(), BOTH16, VST_ATT_PADDED16},
    {"bf16, p = 0.3: the plan does not read p", call(256, 4, 1, 1025, BF16, false, false, 0, 0.3f), defaults(), BOTH16, VST_ATT_PADDED16},
    {"bf16 Linears alone", call(256, 4, 2, 1000, LIN), defaults(), LINEAR16, VST_ATT_PADDED_EXACT},
    {"bf16 attention alone", call(256, 4, 2, 1000, ATT), defaults(), ATTENTION16, VST_ATT_PADDED16},
    {"fp16", call(256, 4, 2, 1000, BF16 | FP16), defaults(), FP16_BOTH, VST_ATT_PADDED16},
    {"fp16 Linears alone", call(256, 4, 2, 1000, LIN | FP16), defaults(), FP16_LINEAR, VST_ATT_PADDED_EXACT},
    {"fp16 attention alone", call(256, 4, 2, 1000, ATT | FP16), defaults(), FP16_ATTENTION, VST_ATT_PADDED16},
    {"fp16 flag alone: exact", call(256, 4, 2, 1000, FP16), defaults(), EXACT, VST_ATT_PADDED_EXACT},
    {"padded calls do not read the packed opt-in", call(256, 4, 2, 1000, BF16 | OPT_IN), defaults(), BOTH16, VST_ATT_PADDED16},
    // the A-stationary kernels: by themselves from 192 * 256 rows, bf16 only
    {"bf16 below 192 * 256 rows", call(256, 4, 3, R16 / 3 - 1, BF16), defaults(), BOTH16, VST_ATT_PADDED16},
    {"bf16 at 192 * 256 rows: rows16", call(256, 4, 48, 1024, BF16), defaults(), BOTH16_ROWS, VST_ATT_PADDED16},
    {"bf16 at 192 * 256 rows, backward: t16", backward(call(256, 4, 48, 1024, BF16)), defaults(), BOTH16_ROWS, VST_ATT_PADDED16},
    {"bf16 Linears alone at 192 * 256 rows: fc1 only", call(256, 4, 48, 1024, LIN), defaults(), LINEAR16_ROWS, VST_ATT_PADDED_EXACT},
    {"fp16 at 192 * 256 rows: tiled", call(256, 4, 48, 1024, BF16 | FP16), defaults(), FP16_BOTH, VST_ATT_PADDED16},
    {"d 512 (K = 512) at 192 * 256 rows: rows16", call(512, 8, 48, 1024, BF16), defaults(), BOTH16_ROWS, VST_ATT_PADDED16},
    {"d 1024 at 192 * 256 rows: no A-stationary kernel", call(1024, 8, 48, 1024, BF16), defaults(), BOTH16, VST_ATT_PADDED16},
    // head dims
    {"head dim 32", call(256, 8, 2, 1000, BF16), defaults(), BOTH16, VST_ATT_PADDED16},
    {"head dim 128", call(512, 4, 2, 1000, BF16), defaults(), BOTH16, VST_ATT_PADDED16},
    {"head dim 256: no 16-bit attention", call(256, 1, 2, 1000, BF16), defaults(), LINEAR16, VST_ATT_PADDED_EXACT},
    {"head dim 256, attention flag alone: exact", call(256, 1, 2, 1000, ATT), defaults(), EXACT, VST_ATT_PADDED_EXACT},
    // packed ragged batches
    {"packed, exact", call(256, 4, 1, 2000, 0, true), defaults(), EXACT, VST_ATT_PACKED_EXACT},
    {"packed, bf16 without the opt-in: exact attention", call(256, 4, 1, 2000, BF16, true), defaults(), LINEAR16, VST_ATT_PACKED_EXACT},
    {"packed, bf16 with the opt-in", call(256, 4, 1, 2000, BF16 | OPT_IN, true), defaults(), PACKED_BOTH16, VST_ATT_PACKED16},
    {"packed, bf16 with the opt-in, backward", backward(call(256, 4, 1, 2000, BF16 | OPT_IN, true)), defaults(), PACKED_BOTH16, VST_ATT_PACKED16},
    {"packed, fp16 with the opt-in", call(256, 4, 1, 2000, BF16 | FP16 | OPT_IN, true), defaults(), FP16_PACKED, VST_ATT_PACKED16},
    {"packed, attention alone with the opt-in", call(256, 4, 1, 2000, ATT | OPT_IN, true), defaults(), ATTENTION16, VST_ATT_PACKED16},
    {"packed, opt-in at train_lp_min_rows: exact", call(256, 4, 1, 1024, BF16 | OPT_IN, true), defaults(), EXACT, VST_ATT_PACKED_EXACT},
    {"packed, opt-in, head dim 256", call(256, 1, 1, 2000, BF16 | OPT_IN, true), defaults(), LINEAR16, VST_ATT_PACKED_EXACT},
    {"packed beyond max_len rows (its T is all frames)", call(256, 4, 1, 30000, 0, true), defaults(), EXACT, VST_ATT_PACKED_EXACT},
    // the switches, pinned as the GPU tests do
    {"VS_TRAIN_LP_MIN_ROWS=0: bf16 at 65 rows", call(256, 4, 1, 65, BF16), with(&VskOptions::train_lp_min_rows, 0), BOTH16, VST_ATT_PADDED16},
    {"VS_LP_STORE32: fp32 storage", call(256, 4, 2, 1000, BF16), with(&VskOptions::lp_store32, 1), BOTH_STORE32, VST_ATT_PADDED16},
    {"VS_LP_STORE32, fp16", call(256, 4, 2, 1000, BF16 | FP16), with(&VskOptions::lp_store32, 1), FP16_STORE32, VST_ATT_PADDED16},
    {"VS_LP_MLP_UNFUSED=1 at 192 * 256 rows: tiled", call(256, 4, 48, 1024, BF16), with(&VskOptions::lp_mlp_unfused, 1), BOTH16, VST_ATT_PADDED16},
    {"VS_LP_MLP_UNFUSED=2 at 2000 rows: rows16", call(256, 4, 2, 1000, BF16), with(&VskOptions::lp_mlp_unfused, 2), BOTH16_ROWS, VST_ATT_PADDED16},
    {"VS_LP_MLP_UNFUSED=2, d 128: no A-stationary kernel", call(128, 4, 2, 1000, BF16), with(&VskOptions::lp_mlp_unfused, 2), BOTH16, VST_ATT_PADDED16},
    // a handed-back form wins over what the backward would derive (here: exact, the switch having moved since the forward)
    {"backward, reserved = bf16 form at 65 rows", backward(call(256, 4, 1, 65, BF16), 0x8000000fu), defaults(), BOTH16, VST_ATT_PADDED16},
    {"backward, reserved = rows16 form at 65 rows", backward(call(256, 4, 1, 65, BF16), 0x8000001fu), defaults(), BOTH16_ROWS, VST_ATT_PADDED16},
    {"backward, reserved = exact form under bf16 flags", backward(call(256, 4, 2, 1000, BF16), 0x80000000u), defaults(), EXACT, VST_ATT_PADDED_EXACT},
    {"forward ignores reserved", call(256, 4, 2, 1000, 0, false, false, 0x8000000fu), defaults(), EXACT, VST_ATT_PADDED_EXACT},
    {"backward, reserved without bit 31: derived", backward(call(256, 4, 2, 1000, BF16), 0x00000004u), defaults(), BOTH16, VST_ATT_PADDED16},
};

// ---- part 2: each switch against its base case ("acts on") ----
struct Flip { const char *name; int VskOptions::*field; int value; VsTrainIn in; unsigned fields; };
const VsTrainIn BIG = call(256, 4, 48, 1024, BF16), MID = call(256, 4, 2, 1000, BF16), SMALL = call(256, 4, 1, 65, BF16);
const Flip kFlips[] = {
    {"VS_LP_STORE32", &VskOptions::lp_store32, 1, BIG,
     FORM_STORAGE | bit(F_ROWS16) | bit(F_FORMAT) | bit(F_KV_STRIDE) | bit(F_QKV_ROWS16) | bit(F_FAMILIES) | MODES_QKV | MODES_HIDDEN},
    {"VS_LP_STORE32, backward", &VskOptions::lp_store32, 1, backward(BIG),
     FORM_STORAGE | bit(F_ROWS16) | bit(F_FORMAT) | bit(F_KV_STRIDE) | bit(F_QKV_ROWS16) | bit(F_T16) | MODES_QKV | MODES_HIDDEN},
    {"VS_LP_STORE32 below 192 * 256 rows", &VskOptions::lp_store32, 1, MID, FORM_STORAGE | bit(F_FORMAT) | bit(F_KV_STRIDE) | MODES_QKV | MODES_HIDDEN},
    {"VS_LP_MLP_UNFUSED=1", &VskOptions::lp_mlp_unfused, 1, BIG, bit(F_ROWS16) | bit(F_FORMAT) | bit(F_QKV_ROWS16) | bit(F_FAMILIES)},
    {"VS_LP_MLP_UNFUSED=1, backward", &VskOptions::lp_mlp_unfused, 1, backward(BIG), bit(F_ROWS16) | bit(F_FORMAT) | bit(F_QKV_ROWS16) | bit(F_T16)},
    {"VS_LP_MLP_UNFUSED=1 below 192 * 256 rows", &VskOptions::lp_mlp_unfused, 1, MID, 0u},
    {"VS_LP_MLP_UNFUSED=2", &VskOptions::lp_mlp_unfused, 2, MID, bit(F_ROWS16) | bit(F_FORMAT) | bit(F_QKV_ROWS16) | bit(F_FAMILIES)},
    {"VS_LP_MLP_UNFUSED=2, backward", &VskOptions::lp_mlp_unfused, 2, backward(MID), bit(F_ROWS16) | bit(F_FORMAT) | bit(F_QKV_ROWS16) | bit(F_T16)},
    {"VS_LP_MLP_UNFUSED=2 from 192 * 256 rows", &VskOptions::lp_mlp_unfused, 2, BIG, 0u},
    {"VS_TRAIN_LP_MIN_ROWS=0", &VskOptions::train_lp_min_rows, 0, SMALL,
     bit(F_LP) | bit(F_LPA) | FORM_STORAGE | bit(F_FORMAT) | bit(F_ATTENTION) | bit(F_KV_STRIDE) | bit(F_LINEAR) | MODES_QKV | MODES_HIDDEN},
    {"VS_TRAIN_LP_MIN_ROWS=0 above 1024 rows", &VskOptions::train_lp_min_rows, 0, MID, 0u},
    // a backward that is handed the forward's form reads no switch
    {"VS_LP_STORE32, backward with the form", &VskOptions::lp_store32, 1, backward(BIG, 0x8000001fu), 0u},
    {"VS_LP_MLP_UNFUSED=1, backward with the form", &VskOptions::lp_mlp_unfused, 1, backward(BIG, 0x8000001fu), 0u},
    {"VS_TRAIN_LP_MIN_ROWS=0, backward with the form", &VskOptions::train_lp_min_rows, 0, backward(SMALL, 0x80000000u), 0u},
};

// ---- the parent's rules, spelled out once more for the test ----
bool dh_has_16bit_attention(int dh) { return dh == 32 || dh == 64 || dh == 128; }
bool a_stationary_fc1_exists(int d) { return d == 256 || d == 512; }       // K = d, N = 4 d <= 4096
// vs_dropout_cfg.reserved (bit 31 set) that a backward refuses
bool form_word_refused(unsigned fb, const VsTrainIn &in) {
    const bool lp = fb & 1u, lpa = fb & 2u, qkv16 = fb & 4u, h16 = fb & 8u, rows16 = fb & 16u, f16 = fb & 32u;
    return (qkv16 && !(lp && lpa)) || (h16 && !lp) || (rows16 && !h16) || (f16 && (rows16 || !(lp || lpa))) || (fb & 0x7fffffc0u) || (in.packed && qkv16) ||
           (lpa && !dh_has_16bit_attention(in.d_model / in.num_heads)) || (rows16 && !a_stationary_fc1_exists(in.d_model));
}
std::string form_refusal_text(unsigned fb) {
    char msg[128];
    snprintf(msg, sizeof msg, "vs_dropout_cfg.reserved = 0x%08x is not a record form this model / batch can have", fb);
    return msg;
}

const int kDims[][2] = {{128, 4}, {256, 8}, {256, 4}, {256, 2}, {256, 1}, {320, 5}, {512, 16}, {512, 8}, {512, 4}, {512, 2}, {1024, 8}, {1024, 4}};   // head dim 32 .. 256
const int kBT[][2] = {{1, 8}, {1, 65}, {5, 13}, {1, 1024}, {1, 1025}, {5, 205}, {4, 4096}, {1, 16385}, {48, 1023}, {48, 1024}, {64, 1024}};

// ---- part 3: invariants over shapes x flags x switches x padded / packed x direction ----
int grid(long long *points, std::set<std::pair<int, long long>> *reached) {
    for (auto &dm : kDims) for (auto &s : kBT) for (unsigned flags = 0; flags < 16; ++flags) for (int store32 = 0; store32 < 2; ++store32)
        for (int unfused = 0; unfused < 3; ++unfused) for (int min0 = 0; min0 < 2; ++min0) for (int pk = 0; pk < 2; ++pk) {
            VskOptions opt = defaults();
            opt.lp_store32 = store32; opt.lp_mlp_unfused = unfused;
            if (min0) opt.train_lp_min_rows = 0;
            const VsTrainIn fwd = call(dm[0], dm[1], s[0], s[1], flags, pk != 0);
            const int M = fwd.B * fwd.T, dh = dm[0] / dm[1];
            VsTrainPlan p, b0, bf, other;
            std::string err;
            CHECK(vs_train_plan(fwd, opt, &p, &err) == VS_OK && err.empty());
            // the backward: deriving again under the same switches, or handed the form back - under these switches or any others
            CHECK(vs_train_plan(backward(fwd), opt, &b0, &err) == VS_OK);
            CHECK(vs_train_form_possible(p.format, fwd));
            CHECK(vs_train_plan(backward(fwd, p.format), opt, &bf, &err) == VS_OK);
            CHECK(differing(b0, bf) == 0);
            VskOptions flipped = defaults();
            flipped.lp_store32 = !store32; flipped.lp_mlp_unfused = (unfused + 1) % 3; flipped.train_lp_min_rows = min0 ? 1 << 20 : 0;
            CHECK(vs_train_plan(backward(fwd, p.format), flipped, &other, &err) == VS_OK && differing(bf, other) == 0);
            *points += 4;
            // forward and backward differ only in what they ensure
            CHECK((differing(p, b0) & ~(bit(F_FAMILIES) | bit(F_T_FRAGMENTS) | bit(F_T16))) == 0);
            CHECK(!p.transposed_fragments && !p.t16 && b0.families == 0);
            CHECK(p.families == ((M <= opt.skinny_rows ? (unsigned)VSW_FRAGMENTS : 0u) | (p.form.rows16 ? (unsigned)VSW_ROWS16 : 0u)));
            CHECK(b0.transposed_fragments == (M <= opt.skinny_rows) && b0.t16 == p.form.rows16);
            const VsTrainForm &f = p.form;
            CHECK(vs_train_form_parse(p.format) == f && vs_train_form_bits(f) == p.format && (p.format & ~0x8000003fu) == 0);
            CHECK(!f.qkv16 || (f.lp && f.lpa && !pk));
            CHECK(!f.h16 || f.lp);
            CHECK(!f.rows16 || (f.h16 && !f.f16));
            CHECK(!f.f16 || f.lp || f.lpa);
            CHECK(!f.lpa || dh_has_16bit_attention(dh));
            CHECK(!f.rows16 || a_stationary_fc1_exists(dm[0]));
            CHECK(!(f.lp || f.lpa) || M > opt.train_lp_min_rows);
            CHECK(!store32 || !(f.qkv16 || f.h16));
            const size_t plane = (size_t)M * dm[0];
            CHECK(p.kv_stride == (f.qkv16 ? plane / 2 : plane));
            CHECK(p.qkv_rows16 == (f.rows16 && f.qkv16));
            CHECK(p.attention == (pk ? (f.lpa ? VST_ATT_PACKED16 : VST_ATT_PACKED_EXACT) : (f.lpa ? VST_ATT_PADDED16 : VST_ATT_PADDED_EXACT)));
            // each mode word agrees with the storage fact it encodes: a tensor's producer and every consumer of it say the same
            const int fbit = f.f16 ? F : 0;
            // q / k / v: vsk_qkv writes, the attention (both directions) reads
            CHECK(((p.mode_qkv & S) != 0) == f.qkv16 && (p.mode_attention & 1) == (f.qkv16 ? 1 : 0) && (p.mode_attention & ~(1 | F)) == 0);
            // dO: the out-projection's dgrad writes, the row dot and the attention backward (mode_attention) read
            CHECK(((p.mode_datt & S) != 0) == f.qkv16 && ((p.mode_rowdot & 3) == 1) == f.qkv16);
            CHECK(((p.mode_rowdot & 3) == 2) == (f.lpa && !f.qkv16) && ((p.mode_rowdot & 3) == 0) == !f.lpa && (p.mode_rowdot & ~(3 | F)) == 0);
            // dq | dk | dv: the attention backward writes, the QKV wgrad and dgrad read
            CHECK(p.attention_out16 == f.qkv16 && ((p.mode_wgrad_qkv & Y) != 0) == f.qkv16 && ((p.mode_dgrad_qkv & A) != 0) == f.qkv16);
            CHECK(!(p.mode_wgrad_qkv & X) && !(p.mode_qkv & A) && !(p.mode_datt & A) && !(p.mode_dgrad_qkv & S));
            // the MLP hidden tensor: fc1 writes; fc2, W2's wgrad and the gate read
            CHECK(((p.mode_fc1 & S) != 0) == f.h16 && ((p.mode_fc2 & A) != 0) == f.h16 && ((p.mode_wgrad_w2 & X) != 0) == f.h16);
            // its gradient: the gate GEMM writes (stored as the activation it gates is), W1's wgrad and fc1's dgrad read
            CHECK(((p.mode_gate & S) != 0) == f.h16 && ((p.mode_wgrad_w1 & Y) != 0) == f.h16 && ((p.mode_dgrad_fc1 & A) != 0) == f.h16);
            CHECK(!(p.mode_wgrad_w2 & Y) && !(p.mode_wgrad_w1 & X) && !(p.mode_fc1 & A) && !(p.mode_fc2 & S) && !(p.mode_gate & A) && !(p.mode_dgrad_fc1 & S));
            // every GEMM word: bit 0 = the 16-bit pipe, VSK_F16 rides on it; nothing is stored 16-bit by an exact GEMM
            const int gemm[] = {p.mode_linear, p.mode_qkv, p.mode_fc1, p.mode_fc2, p.mode_wgrad_w2, p.mode_gate, p.mode_wgrad_w1, p.mode_dgrad_fc1,
                                p.mode_datt, p.mode_wgrad_qkv, p.mode_dgrad_qkv};
            for (int word : gemm) CHECK((word & 1) == (f.lp ? 1 : 0) && (word & F) == (f.lp ? fbit : 0) && (f.lp || word == 0));
            CHECK(p.mode_linear == (f.lp ? (1 | fbit) : 0));
            CHECK((p.mode_attention & F) == fbit && (p.mode_rowdot & F) == (f.lpa ? fbit : 0));
            long long v[F_COUNT];
            values(p, v); for (int fl = F_ATTENTION; fl < F_COUNT; ++fl) if (fl != F_KV_STRIDE) reached->insert({fl, v[fl]});
            values(b0, v); for (int fl = F_ATTENTION; fl < F_COUNT; ++fl) if (fl != F_KV_STRIDE) reached->insert({fl, v[fl]});
        }
    return 0;
}

// ---- part 4: every form word a caller can hand back ----
int form_words(long long *points) {
    for (auto &dm : kDims) for (auto &s : kBT) for (int pk = 0; pk < 2; ++pk) for (int stray = -1; stray < 31; ++stray) {
        if (stray >= 0 && stray < 6) continue;
        for (unsigned low = 0; low < 64; ++low) {
            const unsigned fb = 0x80000000u | low | (stray >= 0 ? 1u << stray : 0u);
            const VsTrainIn in = backward(call(dm[0], dm[1], s[0], s[1], BF16, pk != 0), fb);
            VsTrainPlan p, untouched;
            std::memset((void *)&p, 0x5a, sizeof p);
            std::memcpy((void *)&untouched, (const void *)&p, sizeof p);
            std::string err;
            const int rc = vs_train_plan(in, defaults(), &p, &err);
            ++*points;
            if (form_word_refused(fb, in)) {
                CHECK(rc == VS_ERR_INVALID && err == form_refusal_text(fb) && std::memcmp((const void *)&p, (const void *)&untouched, sizeof p) == 0);
                CHECK(!vs_train_form_possible(fb, in));
                continue;
            }
            CHECK(rc == VS_OK && err.empty() && p.format == fb && vs_train_form_bits(p.form) == fb && vs_train_form_possible(fb, in));
            // the same word in a forward's config is not read
            VsTrainIn f = in;
            f.backward = false;
            VsTrainPlan pf, pf0;
            CHECK(vs_train_plan(f, defaults(), &pf, &err) == VS_OK);
            f.reserved = 0;
            CHECK(vs_train_plan(f, defaults(), &pf0, &err) == VS_OK && differing(pf, pf0) == 0);
        }
    }
    return 0;
}

}  // namespace

int main() {
    for (const Case &c : kCases) CHECK(plan_is(c));

    for (const Flip &f : kFlips) {
        VsTrainPlan a, b;
        std::string err;
        CHECK(vs_train_plan(f.in, defaults(), &a, &err) == VS_OK && vs_train_plan(f.in, with(f.field, f.value), &b, &err) == VS_OK);
        if (differing(a, b) != f.fields) { std::printf("FAILED: %s flips fields 0x%x, documented 0x%x\n", f.name, differing(a, b), f.fields); return 1; }
    }

    long long points = 0;
    std::set<std::pair<int, long long>> reached;
    if (grid(&points, &reached)) return 1;
    // the named cases reach every attention kernel and every value of every ensure field and mode word that the grid reaches
    for (int a = VST_ATT_PACKED16; a <= VST_ATT_PADDED_EXACT; ++a) CHECK(g_seen.count({F_ATTENTION, a}) == 1);
    for (const auto &fv : reached)
        if (!g_seen.count(fv)) { std::printf("FAILED: no named case gives field %d the value %lld\n", fv.first, fv.second); return 1; }
    if (form_words(&points)) return 1;

    {   // part 5: the argument refusals: code, text, order of precedence
        VsTrainPlan p, untouched;
        std::memset((void *)&p, 0x5a, sizeof p);
        std::memcpy((void *)&untouched, (const void *)&p, sizeof p);
        std::string err;
        auto refused = [&](VsTrainIn in, const char *text) {
            err.clear();
            std::memcpy((void *)&p, (const void *)&untouched, sizeof p);
            return vs_train_plan(in, defaults(), &p, &err) == VS_ERR_INVALID && err == text && std::memcmp((const void *)&p, (const void *)&untouched, sizeof p) == 0;
        };
        VsTrainIn in = backward(call(256, 4, 0, -1, BF16), 0x80000004u);      // every rule at once: the first one speaks
        in.max_len = -5; in.p = 1.f; in.p_embed = -0.5f;
        CHECK(refused(in, "B=0 T=-1"));
        in.B = 3; in.T = 0;
        CHECK(refused(in, "B=3 T=0"));
        in.B = 1 << 15; in.T = 1 << 14;
        CHECK(refused(in, "B*T too large"));
        in.B = 2; in.T = 20001; in.max_len = 20000;
        CHECK(refused(in, "T=20001 exceeds the positional table (max_len=20000)"));
        in.T = 20000;
        CHECK(refused(in, "dropout probabilities must be in [0, 1): p=1 p_embed=-0.5"));
        in.p = 0.25f;
        CHECK(refused(in, "dropout probabilities must be in [0, 1): p=0.25 p_embed=-0.5"));
        in.p = -0.125f; in.p_embed = 0.f;
        CHECK(refused(in, "dropout probabilities must be in [0, 1): p=-0.125 p_embed=0"));
        in.p = 0.f; in.p_embed = 1.f;
        CHECK(refused(in, "dropout probabilities must be in [0, 1): p=0 p_embed=1"));
        in.p_embed = 0.5f;
        CHECK(refused(in, "vs_dropout_cfg.reserved = 0x80000004 is not a record form this model / batch can have"));
        in.reserved = 0x80000040u;
        CHECK(refused(in, "vs_dropout_cfg.reserved = 0x80000040 is not a record form this model / batch can have"));
        in.reserved = 0;
        CHECK(vs_train_plan(in, defaults(), &p, &err) == VS_OK);
        // T against max_len: padded calls with a positional table only
        VsTrainIn longer = call(256, 4, 1, 20001, 0);
        CHECK(refused(longer, "T=20001 exceeds the positional table (max_len=20000)"));
        longer.has_pe = false;
        CHECK(vs_train_plan(longer, defaults(), &p, &err) == VS_OK);
        CHECK(vs_train_plan(call(256, 4, 1, 20001, 0, true), defaults(), &p, &err) == VS_OK);
        // B * T == 2^28 is the last size taken
        VsTrainIn huge = call(256, 4, 1 << 14, 1 << 14, 0);
        CHECK(vs_train_plan(huge, defaults(), &p, &err) == VS_OK);
        huge.B += 1;
        CHECK(refused(huge, "B*T too large"));
    }

    std::printf("OK\n");
    return 0;
}
