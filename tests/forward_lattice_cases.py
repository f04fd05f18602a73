"""The scoring forward's whole native space at tiny sizes, shared by tests/test_forward_lattice_host.py (the table against
simnet.embedding_plan) and tests/test_hip_forward_lattice.py (every shape in every compute mode and call form on the GPU).

The space is native shape x compute mode x call form.  NATIVE is every (heads, d_model) the kernels run as it is - d_model a
multiple of 64 up to 1024 with head dim 32 / 64 / 128 / 256, exactly where embedding_plan returns None: 44 shapes.  Small enough
to walk, so nothing is drawn at random: the planner (csrc/vs_forward_plan.h) picks kernels from d_model (<= 256, == 256, above),
the head dim and the row count, and each of those splits appears under every head dim the arithmetic allows.

The batch: four videos of 130, 1, 33 and 257 frames (421 rows) - a one-frame video, and lengths either side of the 32-row wave
tile and of the 128- and 256-row block tiles - padded to [4, 257, 1024] with synth.padding_mask, or packed.  Two layers, so a
kernel that carries the next layer's QKV has a middle and a last layer.  Each cell runs with the row thresholds pinned to 0
(the tiled and bf16 kernels at these row counts) and at their defaults (the latency kernels).

Latency mode (set_latency_mode) is walked over embedding widths separately: one 65-frame video, in_features 1024 / 2048 / 3072 -
an eighth of 3072 is not a K slice the split-K kernel takes - at d_model 128 / 256 / 512.
"""
HEAD_DIMS = (32, 64, 128, 256)
NATIVE = tuple((d // dh, d) for d in range(64, 1025, 64) for dh in HEAD_DIMS if d % dh == 0)       # (num_heads, d_model)
NATIVE_COUNT = 44

LENGTHS = (130, 1, 33, 257)
ROWS = sum(LENGTHS)
NUM_LAYERS = 2
IN_FEATURES = 1024
MODES = ("fp32", "fp16x3", "bf16")
PIN_OPTIONS = ("VS_SKINNY_ROWS", "VS_LP_MIN_ROWS")
PINS = (0, -1)                                  # both thresholds at 0, then both at their defaults
PACKED_HEAD_DIMS = (32, 64, 128)                # forward_packed / score_packed; head dim 256 is refused with a message
PACKED_REFUSAL = "packed batches need head_dim 32, 64 or 128 (got 256)"

LATENCY_MODELS = ((4, 128), (4, 256), (4, 512))     # (num_heads, d_model): head dim 32, 64, 128
LATENCY_IN_FEATURES = (1024, 2048, 3072)
LATENCY_FRAMES = 65
LATENCY_MODES = ("fp32", "fp16x3")


def shape_id(shape):
    return "h%d_d%d" % shape


def seeds(shape):
    """(weights, features): one fixed pair per shape"""
    H, d = shape
    return 9000 + 16 * d + H, 9001 + 16 * d + H


def latency_seeds(shape, in_features):
    H, d = shape
    return 12000 + 16 * d + in_features // 64, 12001 + 16 * d + in_features // 64
