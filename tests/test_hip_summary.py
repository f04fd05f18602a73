"""GPU: the keyshot summary from device-resident scores (summary.summarize_scores, include/vs_summary.h) against the
reference's goldens (tests/golden/eval_golden.npz, eval_nan_golden.npz) and the host library (evaluation.generate_summary,
upsample, knapSack - pinned to the reference by tests/test_evaluation.py).  Everything that decides a result is the
reference's own float32 / double operation in the reference's order, so "equal" below means np.array_equal: no tolerance.

Every device result comes from ONE raw vs_summarize call per group of videos, made once per module, whose outputs and
workspace lie between guard bands of a sentinel: every test that looks at a result also checks that nothing outside the
outputs was written and that `frames` past n_selected_frames still holds the sentinel."""
import ctypes as C
import importlib
import json
import os
import warnings

import numpy as np
import pytest
import torch

from conftest import GOLDEN

pytestmark = pytest.mark.gpu

G = np.load(os.path.join(GOLDEN, "eval_golden.npz"))
GN = np.load(os.path.join(GOLDEN, "eval_nan_golden.npz"))
LDS_COLS = 2048             # csrc/vs_eval_device_kernels.h EV_LDS_COLS: knapsack rows of more columns live in the workspace
LDS_BITS = 3072             # ... EV_LDS_BITS: more 64-bit words of change bits (n_shots * ceil((W + 1) / 64)) live there too
PASS = 256                  # ... EV_NT: knapsack columns per pass, threads per block, shots per pass of the scan
FILL_TILE = 1024            # csrc/vs_summary_kernels.h SM_FILL_TILE: summary bytes per block of summary_fill
GUARD = 512                 # guard band, in elements, on either side of every device buffer
SENT8, SENT32 = -86, -1234567


class Rec:
    def __init__(self, **kw):
        self.__dict__.update(kw)


class Video:
    """One video as vs_summarize takes it."""

    def __init__(self, scores, cps, n_frames, picks):
        self.scores = np.ascontiguousarray(scores, dtype=np.float32)
        self.cps = np.ascontiguousarray(np.asarray(cps).reshape(-1, 2), dtype=np.int32)
        self.n_frames = int(n_frames)
        self.picks = np.ascontiguousarray(picks, dtype=np.int32).reshape(-1)
        self.L = int(self.cps[-1, 1]) + 1


def _dev():
    assert torch.cuda.is_available(), "these tests need a HIP device"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def mods(vsa):
    vsa._lib.build()
    return Rec(vsa=vsa, L=vsa._lib, ev=importlib.import_module("video-summarization_amd.evaluation"),
               sm=importlib.import_module("video-summarization_amd.summary"))


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def _guarded(n, dtype, sentinel, dev, lead=0):
    """A device buffer of n elements between two guard bands; `lead` extra elements shift its start (alignment cases)."""
    whole = torch.full((GUARD + lead + n + GUARD,), sentinel, dtype=dtype, device=dev)
    return whole, whole[GUARD + lead: GUARD + lead + n]


def _raw(mods, videos, proportion=0.15, lead=0):
    """ONE vs_summarize call over `videos` -> Rec(summary, frames, n_sel, sel, means: per-video lists; guards_intact,
    tail_untouched: what the call left alone)."""
    L, lib, dev = mods.L, mods.L.load(), _dev()
    i32 = lambda v: np.ascontiguousarray(v, dtype=np.int32)
    nsc, npos = i32([v.scores.size for v in videos]), i32([v.picks.size for v in videos])
    nf, nsh = i32([v.n_frames for v in videos]), i32([v.cps.shape[0] for v in videos])
    pos, cps = np.concatenate([v.picks for v in videos]), np.ascontiguousarray(np.concatenate([v.cps for v in videos]))
    scores = torch.from_numpy(np.concatenate([v.scores for v in videos])).to(dev)
    lens = [v.L for v in videos]
    total = sum(lens)
    need = lib.vs_summarize_workspace_bytes(len(videos), _p(npos), _p(nf), _p(nsh), _p(cps), float(proportion))
    assert need > 0, lib.vs_last_error()
    s_whole, summary = _guarded(total, torch.int8, SENT8, dev, lead)
    f_whole, frames = _guarded(total, torch.int32, SENT32, dev)
    w_whole = torch.full((need + 2 * 256 * 3,), 0x5A, dtype=torch.uint8, device=dev)
    at = 256 + (-w_whole.data_ptr()) % 256                      # a 256-byte aligned workspace with >= 256 guard bytes around it
    ws = w_whole[at: at + need]
    n_sel = np.full(len(videos), -7, dtype=np.int32)
    sel = np.full(int(nsh.sum()), -7, dtype=np.int8)
    means = np.full(int(nsh.sum()), -7.0, dtype=np.float64)
    stream = torch.cuda.current_stream(dev).cuda_stream
    rc = lib.vs_summarize(len(videos), _p(nsc), _p(npos), _p(nf), _p(nsh), _p(pos), _p(cps), float(proportion),
                          C.c_void_p(scores.data_ptr()), C.c_void_p(summary.data_ptr()), C.c_void_p(frames.data_ptr()), _p(n_sel),
                          _p(sel), _p(means), C.c_void_p(ws.data_ptr()), need, C.c_void_p(stream))
    assert rc == L.VS_OK, lib.vs_last_error()
    s_host, f_host, w_host = s_whole.cpu().numpy(), f_whole.cpu().numpy(), w_whole.cpu().numpy()
    guards = bool((s_host[: GUARD + lead] == SENT8).all() and (s_host[GUARD + lead + total:] == SENT8).all()
                  and (f_host[:GUARD] == SENT32).all() and (f_host[GUARD + total:] == SENT32).all()
                  and (w_host[:at] == 0x5A).all() and (w_host[at + need:] == 0x5A).all())
    s_host, f_host = s_host[GUARD + lead: GUARD + lead + total], f_host[GUARD: GUARD + total]
    out = Rec(summary=[], frames=[], n_sel=n_sel, sel=[], means=[], guards_intact=guards, tail_untouched=True, offsets=[])
    o = so = 0
    for v, k in zip(videos, range(len(videos))):
        out.offsets.append(o)
        out.summary.append(s_host[o: o + v.L].copy())
        out.frames.append(f_host[o: o + n_sel[k]].copy())
        out.tail_untouched = out.tail_untouched and bool((f_host[o + n_sel[k]: o + v.L] == SENT32).all())
        out.sel.append(sel[so: so + v.cps.shape[0]].copy())
        out.means.append(means[so: so + v.cps.shape[0]].copy())
        o += v.L
        so += v.cps.shape[0]
    return out


def _restate(ev, v, proportion=0.15):
    """(summary, selected, means) from host functions only: upsample, float32 np.mean per shot over the clipped range,
    knapSack(int(L * p), unclipped lengths, means), the summary's frames (generate_summary.py:41-55)."""
    fs = ev.upsample(v.scores, v.n_frames, v.picks)
    nf = v.n_frames
    means = np.empty(v.cps.shape[0], dtype=np.float64)
    with warnings.catch_warnings(), np.errstate(all="ignore"):
        warnings.simplefilter("ignore")
        for s, (a, b) in enumerate(v.cps.tolist()):
            lo = max(0, min(a, nf))
            means[s] = np.float64(np.mean(fs[lo: max(lo, min(b + 1, nf))]))          # float32 mean; an empty slice: NaN
    wt = (v.cps[:, 1] - v.cps[:, 0] + 1).astype(np.int32)
    picked = ev.knapSack(int(float(v.L) * proportion), wt, means, len(wt))
    sel = np.zeros(len(wt), dtype=np.int8)
    sel[picked] = 1
    summary = np.zeros(v.L, dtype=np.int8)
    for s in picked:
        summary[max(0, int(v.cps[s, 0])): min(v.L - 1, int(v.cps[s, 1])) + 1] = 1
    return summary, sel, means


def _host_summary(ev, v):
    return ev.generate_summary([v.cps], [v.scores], [v.n_frames], [v.picks])[0]


def _eqn(a, b):
    return np.array_equal(np.asarray(a), np.asarray(b), equal_nan=True)


def _check_video(ev, run, k, v, proportion=0.15):
    """Video k of a run against the host: the summary, the frames, the count, the selection and the means."""
    summary, sel, means = _restate(ev, v, proportion)
    if proportion == 0.15:
        assert np.array_equal(summary, _host_summary(ev, v))                              # the yardsticks agree
    assert run.summary[k].dtype == np.int8 and np.array_equal(run.summary[k], summary)
    assert np.array_equal(run.frames[k], np.flatnonzero(summary)) and run.n_sel[k] == int(summary.sum())
    assert np.array_equal(run.sel[k], sel) and _eqn(run.means[k], means)
    assert run.guards_intact and run.tail_untouched


# ---- the reference's goldens -------------------------------------------------------------------------------------------
def _golden(i):
    return Video(G["v%d_scores" % i], G["v%d_cps" % i], int(G["v%d_nframes" % i]), G["v%d_picks" % i])


@pytest.fixture(scope="module")
def golden_run(mods):
    videos = [_golden(i) for i in range(5)]
    return videos, _raw(mods, videos)


def test_reference_goldens(mods, golden_run):
    """The five reference videos in one call (n_frames 2211-9534, 19-80 shots)."""
    videos, run = golden_run
    for i, v in enumerate(videos):
        want = G["v%d_summary" % i]
        assert np.array_equal(run.summary[i], want)
        assert np.array_equal(run.frames[i], np.flatnonzero(want))
        assert run.n_sel[i] == np.flatnonzero(want).size
        _check_video(mods.ev, run, i, v)


def test_no_stray_writes(golden_run):
    """Guard bands of a sentinel before and after summary, frames and the workspace are intact after the goldens call, and
    in frames the entries past n_selected_frames[v] of each slice still hold the sentinel."""
    videos, run = golden_run
    assert run.guards_intact
    assert run.tail_untouched
    assert all(0 < run.n_sel[i] < v.L for i, v in enumerate(videos))


def test_shots_past_n_frames_select_like_the_reference(mods):
    """The NaN corner: change points past n_frames average an empty slice (NaN shot means), and Python's max() keeps or
    drops a NaN by position."""
    videos = [Video(GN["v%d_scores" % j], GN["v%d_cps" % j], int(GN["v%d_nframes" % j]), GN["v%d_picks" % j]) for j in range(4)]
    run = _raw(mods, videos)
    for j, v in enumerate(videos):
        assert np.array_equal(run.summary[j], GN["v%d_summary" % j])
        nan_shots = v.cps[:, 0] >= v.n_frames                       # the mean runs over an empty slice
        assert nan_shots.any() and np.array_equal(np.isnan(run.means[j]), nan_shots)
        _check_video(mods.ev, run, j, v)


def test_a_video_does_not_depend_on_its_batch(mods, golden_run):
    videos, run = golden_run
    perm = [3, 0, 4, 2, 1]
    permuted = _raw(mods, [videos[i] for i in perm])
    at = 0
    for i, v in enumerate(videos):
        assert run.offsets[i] == at                                 # video v sits at the sum of the earlier summaries' lengths
        at += v.L
        alone = _raw(mods, [v])
        k = perm.index(i)
        for name in ("summary", "frames", "sel", "means"):
            assert _eqn(getattr(alone, name)[0], getattr(run, name)[i]), (name, i)
            assert _eqn(getattr(permuted, name)[k], getattr(run, name)[i]), (name, i)
        assert alone.n_sel[0] == run.n_sel[i] == permuted.n_sel[k]
        assert alone.guards_intact and alone.tail_untouched
    assert permuted.offsets == list(np.cumsum([0] + [videos[i].L for i in perm[:-1]]))
    assert permuted.guards_intact and permuted.tail_untouched


# ---- edges: small synthetic videos, each group in one call -----------------------------------------------------------------
def _cuts(rng, n_frames, n_cuts):
    cuts = np.sort(rng.choice(np.arange(1, n_frames), size=n_cuts, replace=False)) if n_cuts else np.array([], dtype=np.int64)
    return np.stack([np.concatenate([[0], cuts]), np.concatenate([cuts - 1, [n_frames - 1]])], axis=1)


def _video(rng, n_frames, picks=None, cps=None, scores=None, n_scores=None, n_cuts=None):
    picks = np.arange(0, n_frames, 15) if picks is None else np.asarray(picks)
    if cps is None:
        cps = _cuts(rng, n_frames, min(max(1, n_frames // 120), max(n_frames - 1, 0)) if n_cuts is None else n_cuts)
    n_scores = len(picks) if n_scores is None else n_scores
    sc = rng.random(n_scores).astype(np.float32) if scores is None else scores
    return Video(sc, cps, n_frames, picks)


def _lengths_video(rng):
    """Shots of length 1, 7, 8, 9, 127, 128, 129, 136, 257 and 1025 in one video: every branch of numpy's pairwise sum.
    Picks every 15 frames, random float32 scores: the shots' frames hold runs of 15 equal values."""
    lens = [1, 7, 8, 9, 127, 128, 129, 136, 257, 1025]
    ends = np.cumsum(lens)
    return _video(rng, int(ends[-1]), cps=np.stack([ends - lens, ends - 1], axis=1))


def _edge_cases():
    rng = np.random.default_rng(4242)
    c = {}
    # pick expansion
    c["picks_end_at_n_frames"] = _video(rng, 60, picks=[0, 15, 30, 45, 60], n_cuts=9)          # nothing appended
    c["picks_start_late"] = _video(rng, 60, picks=[7, 20, 40], n_cuts=9)                         # the leading frames are 0
    c["repeated_picks"] = _video(rng, 60, picks=[0, 15, 15, 30, 30, 30, 45], n_cuts=9)           # empty segments
    c["last_segment_is_0"] = _video(rng, 70, picks=[0, 15, 30, 45], n_scores=3, n_cuts=11)       # n_scores == n_positions - 1
    c["pick_beyond_n_frames"] = _video(rng, 60, picks=[0, 20, 40, 90], n_cuts=9)                 # clipped
    c["single_pick"] = _video(rng, 40, picks=[0], n_cuts=7)
    c["n_frames_1"] = _video(rng, 1, picks=[0], cps=[[0, 0]])                                    # W = 0
    c["n_frames_7"] = _video(rng, 7, picks=[0], cps=[[0, 3], [4, 6]])                            # W = 1: no shot fits
    # pairwise sum
    c["shot_lengths"] = _lengths_video(rng)
    # knapsack: W + 1 = 256 (one pass), 257 (two), 2048 (the last LDS row), 2049 (the first row in the workspace)
    for nf, cols in ((1700, PASS), (1707, PASS + 1), (13647, LDS_COLS), (13654, LDS_COLS + 1)):
        assert int(nf * 0.15) + 1 == cols
        c["knapsack_columns_%d" % cols] = _video(rng, nf)
    c["bits_in_the_workspace"] = _video(rng, 13000)                                               # rows in LDS, bits not
    assert int(13000 * 0.15) + 1 <= LDS_COLS and (13000 // 120 + 1) * ((int(13000 * 0.15) + 64) // 64) > LDS_BITS
    c["every_shot_longer_than_W"] = _video(rng, 300, cps=[[0, 59], [60, 119], [120, 179], [180, 239], [240, 299]])
    c["equal_valued_shots"] = _video(rng, 600, scores=np.full(40, 0.25, dtype=np.float32), n_cuts=30)      # the tie rule
    hot = np.full(14, 0.1, dtype=np.float32)
    hot[0] = hot[-1] = 0.9
    c["first_shot_starts_below_0_last_ends_at_last_end"] = _video(rng, 200, cps=[[-5, 9], [10, 99], [100, 189], [190, 199]], scores=hot)
    # scan and fill: more shots than threads in a block, L not a multiple of the fill tile or of 4, adjacent selected shots;
    # its odd length also puts the next video's slice at an odd byte offset
    lens = rng.integers(1, 4, size=300)
    ends = np.cumsum(lens)
    nf = int(ends[-1])
    c["300_short_shots"] = _video(rng, nf, cps=np.stack([ends - lens, ends - 1], axis=1), picks=np.arange(0, nf, 2))
    c["odd_length"] = _video(rng, 2 * FILL_TILE + 37, n_cuts=200)
    c["after_an_odd_offset"] = _video(rng, FILL_TILE + 2, n_cuts=100)
    return c


@pytest.fixture(scope="module")
def edge_run(mods):
    cases = _edge_cases()
    return list(cases), list(cases.values()), _raw(mods, list(cases.values()), lead=1)      # the summary itself starts at an odd address


@pytest.mark.parametrize("name", list(_edge_cases()))
def test_edges_equal_the_host(mods, edge_run, name):
    names, videos, run = edge_run
    k = names.index(name)
    _check_video(mods.ev, run, k, videos[k])


def test_edges_cover_what_they_claim(mods, edge_run):
    """The cases are only worth their names if the corner is really hit."""
    names, videos, run = edge_run
    at = names.index
    ev = mods.ev
    up = lambda n: ev.upsample(videos[at(n)].scores, videos[at(n)].n_frames, videos[at(n)].picks)
    assert (up("picks_start_late")[:7] == 0).all() and (up("last_segment_is_0")[45:] == 0).all() and (up("last_segment_is_0")[:45] != 0).all()
    for n in ("n_frames_1", "n_frames_7", "every_shot_longer_than_W"):
        assert run.n_sel[at(n)] == 0 and run.summary[at(n)].sum() == 0 and run.frames[at(n)].size == 0
    assert int(1 * 0.15) == 0 and int(7 * 0.15) == 1
    for n in names:
        if n.startswith("knapsack_columns") or n in ("bits_in_the_workspace", "shot_lengths", "equal_valued_shots"):
            assert run.n_sel[at(n)] > 0, n
    k = at("first_shot_starts_below_0_last_ends_at_last_end")
    assert run.sel[k].tolist() == [1, 0, 0, 1] and run.summary[k][:10].all() and run.summary[k][190:].all() and run.n_sel[k] == 20
    k = at("300_short_shots")
    sel = run.sel[k]
    assert videos[k].cps.shape[0] == 300 > PASS and (sel[:-1] & sel[1:]).any() and sel[PASS:].any()      # adjacent; past the first scan pass
    assert videos[k].L % 4 != 0 or videos[at("odd_length")].L % 4 != 0
    assert videos[at("odd_length")].L % 2 == 1 and run.offsets[at("after_an_odd_offset")] % 2 == 1
    assert videos[at("odd_length")].L % FILL_TILE != 0 and videos[at("odd_length")].L > 2 * FILL_TILE
    means = run.means[at("equal_valued_shots")]
    assert (means == means[0]).all()


@pytest.mark.parametrize("proportion", [0.0, 0.3, 1.0])
def test_proportion(mods, proportion):
    v = _golden(3)
    run = _raw(mods, [v], proportion)
    _check_video(mods.ev, run, 0, v, proportion)
    if proportion == 0.0:
        assert run.n_sel[0] == 0
    if proportion == 1.0:
        assert run.sel[0].all() and run.n_sel[0] == v.L


# ---- the Python level --------------------------------------------------------------------------------------------------
def test_summarize_scores_list_equals_concatenated_and_host_tensors_raise(mods, golden_run):
    videos, run = golden_run
    sm, dev = mods.sm, _dev()
    args = ([v.cps for v in videos], [v.n_frames for v in videos], [v.picks for v in videos])
    per = [torch.from_numpy(v.scores).to(dev) for v in videos]
    a = sm.summarize_scores(per, *args)
    b = sm.summarize_scores(torch.cat(per), *args)
    for i, v in enumerate(videos):
        for r in (a[i], b[i]):
            assert r.summary.dtype == torch.int8 and r.frames.dtype == torch.int32 and r.summary.is_cuda and r.frames.is_cuda
            assert np.array_equal(r.summary.cpu().numpy(), run.summary[i]) and np.array_equal(r.frames.cpu().numpy(), run.frames[i])
            assert np.array_equal(r.selected_shots, run.sel[i]) and _eqn(r.shot_means, run.means[i])
            assert r.selected_shots.dtype == np.int8 and r.shot_means.dtype == np.float64
    with pytest.raises(ValueError):
        sm.summarize_scores(torch.cat(per).cpu(), *args)
    with pytest.raises(ValueError):
        sm.summarize_scores([t.cpu() for t in per], *args)
    with pytest.raises(ValueError, match="positions decrease"):                 # the library's message
        sm.summarize_scores(per[:1], args[0][:1], args[1][:1], [videos[0].picks[::-1].copy()])


def _model(vsa):
    m = vsa.SimNet(num_heads=4, d_model=256, num_layers=4, sparsity=0.0, dropout=0.3)
    m.load_state_dict(vsa.synth.make_state_dict(256, 4, 1234), strict=True)
    return m.to(_dev()).eval()


@pytest.fixture(scope="module")
def loader_run(mods):
    """A loader of the five golden records' shapes (features from synth, user records from the golden), get_summary and
    generate_video_summary_json over it, and the reference's recipe done with existing functions."""
    vsa, ev, sm = mods.vsa, mods.ev, mods.sm
    m = _model(vsa)
    names = ["video_22", "video_7", "video_6", "video_11", "video_1"]
    loader = []
    for i, n in enumerate(names):
        T = int(G["v%d_scores" % i].size)
        user = Rec(user_summary=G["v%d_user_summary" % i], user_scores=G["v%d_user_scores" % i], change_points=G["v%d_cps" % i],
                   n_frames=int(G["v%d_nframes" % i]), picks=G["v%d_picks" % i], name=n)
        loader.append((vsa.synth.make_features(1, T, 100 + i, "randn"), torch.zeros(1, T), user))
    got = sm.get_summary(m, loader)
    want = {}
    with torch.no_grad():
        for i, (feature, _, user) in enumerate(loader):                       # generate_summary_image.py:62-78
            pred, _ = m(feature.to(_dev()))
            pred = torch.sigmoid(pred.view(1, -1)).squeeze(0).cpu().numpy()
            s = ev.generate_summary([user.change_points], [pred], [user.n_frames], [user.picks])[0]
            want["video_%d" % i] = np.flatnonzero(s).tolist()
    return m, loader, got, want


def test_get_summary_equals_the_reference_recipe(loader_run):
    _, _, got, want = loader_run
    assert list(got) == list(want) == ["video_%d" % i for i in range(5)]
    assert got == want
    assert all(len(v) > 0 and isinstance(v[0], int) for v in got.values())


def test_generate_video_summary_json_writes_what_get_summary_returns(mods, loader_run, tmp_path, monkeypatch):
    m, loader, got, _ = loader_run
    monkeypatch.chdir(tmp_path)
    mods.sm.generate_video_summary_json(m, loader)
    text = (tmp_path / "summary.json").read_text()
    assert json.loads(text) == got
    assert text == json.dumps(got, indent=8)


def test_summarize_without_change_points_equals_the_composed_steps(mods):
    """summarize(model, features, num_seg=, v_max=) on three synthetic videos (T = 97, 320, 650) against the same steps
    from kts_seg_batch, shots_from_change_points, score and the host generate_summary."""
    vsa, ev, sm = mods.vsa, mods.ev, mods.sm
    seg = vsa.segmentation
    m = _model(vsa)
    T = [97, 320, 650]
    num_seg, v_max = 12, 1.0
    feats = [vsa.synth.make_features(1, t, 300 + t, "randn")[0].to(_dev()) for t in T]
    got = sm.summarize(m, feats, num_seg=num_seg, v_max=v_max)
    cps = seg.kts_seg_batch(feats, [min(num_seg, t - 1) for t in T], v_max)
    assert len(got) == 3
    for i, t in enumerate(T):
        shots = seg.shots_from_change_points(cps[i], t, np.arange(t))
        with torch.no_grad():
            scores = m.score(feats[i][None]).reshape(-1).cpu().numpy()
        want = ev.generate_summary([shots], [scores], [t], [np.arange(t)])[0]
        assert np.array_equal(got[i].summary.cpu().numpy(), want)
        assert np.array_equal(got[i].frames.cpu().numpy(), np.flatnonzero(want))
        assert got[i].selected_shots.size == shots.shape[0] and want.sum() > 0
    with pytest.raises(ValueError):
        sm.summarize(m, feats)                                               # neither change_points nor num_seg
