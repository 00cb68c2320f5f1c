"""CPU, no device: the float64 contracts of tests/attn_ref.py against torch float64 written out independently and
against the oracle's attention functions, and what the GPU comparisons of tests/test_gpu_attn_contract.py rely on for
the same case table:

  * hsp_mha_plan (validation + the one decision function, no launch) returns the kernel and NDB each hsp_mha_f32 case
    id names, with at most 160 KB of LDS,
  * the table reaches every (kernel, NDB) pair the decision function can return (the reachable set is probed from
    hsp_mha_plan itself, not written down here), every kernel in a contiguous and a side-by-side layout, every
    mask-capable kernel with factor, dense and combined masks,
  * the refusals of both entry points, each next to its accepted neighbour,
  * the admission condition of the two bars: for every case the plain float32 numpy evaluation of the contract lies
    within attn_ref.derived_bound (element-wise) and within helpers.tol_for.

The numerical regimes shape the logits through channel 0 of every head: `off` gives every query row a common offset of
+-50..200 (the float64 softmax is the control's; a missing maximum subtraction overflows), `stair{up,dn}{3,30}` steps that
channel of k per key block of the kernel (3: every block matters, 30: one does), `dom` makes one key dominant (the
output is that v column), `v1` sets v to 1 (the output is 1).

    python -m pytest tests/test_attn_ref_host.py -q -s
"""
import ctypes
import itertools

import numpy as np
import pytest
import torch

import attn_ref as R
import helpers as H

RTOL = 1e-12


@pytest.fixture(autouse=True)
def _threads():
    torch.set_num_threads(min(16, torch.get_num_threads()))


@pytest.fixture(scope="module")
def L():
    from megatts2_hierspeechpp_amd import _lib
    _lib.lib()
    return _lib


def _t(x):
    return torch.from_numpy(np.ascontiguousarray(x, dtype=np.float64))


def _views(a):
    """q [B,H,D,Tq], k, v [B,H,D,Tk] as float64 torch tensors (dead keys of a key_len case read as 0)."""
    return tuple(_t(x) for x in R._qkv(a, np.float64))


# ------------------------------------------------------------------------------------------------ contract == torch
def _torch_attention(a, q, k, v, lens=None):
    B, Hh, D, Tq = q.shape
    Tk = k.shape[3]
    w = R.eff(a)[0]
    qs = q * a["qk_scale"]
    s = torch.einsum("bhdi,bhdj->bhij", qs, k)
    if a.get("rel_k") is not None:
        ek, ev = _t(a["rel_k"]).view(2 * w + 1, D), _t(a["rel_v"]).view(2 * w + 1, D)
        for r in range(-w, w + 1):                      # keys j = i + r
            lo, hi = max(0, -r), min(Tq, Tk - r)
            if hi > lo:
                s.diagonal(r, 2, 3)[..., :hi - lo] += torch.einsum("bhdi,d->bhi", qs[..., lo:hi], ek[r + w])
    if a.get("mask_q") is not None:
        mq = torch.from_numpy(a["mask_q"][:B * Tq].reshape(B, Tq))
        mk = torch.from_numpy(a["mask_k"][:B * Tk].reshape(B, Tk))
        s = s.masked_fill((mq[:, None, :, None] * mk[:, None, None, :]) == 0, -1e4)
    if a.get("mask_dense") is not None:
        md = torch.stack([torch.from_numpy(a["mask_dense"][a["mask_dense_off"] + b * a["mask_dense_bs"]:][:Tq * Tk])
                          for b in range(B)]).view(B, 1, Tq, Tk)
        s = s.masked_fill(md == 0, -1e4)
    if lens is None:
        p = torch.softmax(s, dim=-1)
    else:
        p = torch.zeros_like(s)
        for b, n in enumerate(lens):
            p[b, :, :, :n] = torch.softmax(s[b, :, :, :n], dim=-1)
    o = torch.einsum("bhij,bhdj->bhdi", p, v)
    if a.get("rel_k") is not None:
        for r in range(-w, w + 1):
            lo, hi = max(0, -r), min(Tq, Tk - r)
            if hi > lo:
                o[..., lo:hi] += p.diagonal(r, 2, 3)[..., :hi - lo].unsqueeze(2) * ev[r + w].view(1, 1, D, 1)
    return o.reshape(B, Hh * D, Tq)


def _torch_reference(a):
    q, k, v = _views(a)
    if a["entry"] == "mha":
        return _torch_attention(a, q, k, v).numpy()
    B, M, Tq = a["B"], a["M"], a["Tq"]
    o = _torch_attention(a, q, k, v, None if a.get("key_len") is None else
                         [min(max(int(n), 1), a["Tk"]) for n in a["key_len"]])
    wt = _t(a["wt"][:M * a["wt_ld"]].reshape(M, a["wt_ld"])[:, :M])
    y = torch.einsum("mc,bci->bmi", wt, o)
    if a.get("bias") is not None:
        y = y + _t(a["bias"][:M])[None, :, None]
    if a.get("mask") is not None:
        y = y * torch.stack([_t(a["mask"][b * a["mask_bs"]:][:Tq]) for b in range(B)])[:, None, :]
    if a.get("cscale") is not None:
        y = y * torch.stack([_t(a["cscale"][b * a["cscale_bs"]:][:M]) for b in range(B)])[:, :, None]
    if a.get("res") is not None:
        y = y + torch.as_strided(_t(a["res"]), (B, M, Tq), (a["res_bs"], a["res_cs"], a["res_ts"]), a["res_off"])
    return y.numpy()


@pytest.mark.parametrize("id", R.IDS)
def test_contract_equals_torch_float64(id):
    a, ref, written = R.case(id)
    idx = R.out_index(a)
    want = _torch_reference(a)
    err = np.abs(ref[idx] - want) / np.maximum(1.0, np.abs(want))
    assert float(err.max()) <= RTOL, f"{id}: relative difference {err.max():.2e}"
    own = np.zeros(ref.shape, bool)
    own[idx.reshape(-1)] = True
    assert np.array_equal(own, written), id
    buf = a[R.out_name(a)]
    assert (buf[~own] == R.SENT).all() and np.array_equal(ref[~own], buf.astype(np.float64)[~own]), id
    if not a.get("res_is_y"):
        assert (buf == R.SENT).all()
    # every input buffer is poison outside the elements of its operand
    for n in ("q", "k", "v"):
        T = a["Tq"] if n == "q" else a["Tk"]
        ii = R.index(a, n, (a["B"], a["H"] * a["D"], T), (a[n + "_bs"], a[n + "_cs"] or T, 1))
        rest = np.ones(a[n].shape, bool)
        rest[ii.reshape(-1)] = False
        assert rest.any() and np.isnan(a[n][rest]).all(), (id, n)
    reg = a["reg"] if a.get("rel_k") is None else ""       # a window adds its relative-value term to the output
    if a["entry"] == "mha" and reg == "v1":
        assert np.abs(ref[written] - 1.0).max() <= 1e-12
    if a["entry"] == "mha" and reg == "dom" and not a.get("mask"):
        _, _, v = _views(a)
        col = v[..., (2 * a["Tk"]) // 3].reshape(a["B"], -1, 1).numpy()
        assert np.abs(ref[idx] - col).max() <= 1e-6 * max(1.0, np.abs(col).max()), id


def _sd_identity(name, C, kv_from=None):
    eye = torch.eye(C, dtype=torch.float64)
    z = torch.zeros(C, C, dtype=torch.float64)
    return {f"{name}.conv_q.weight": eye[:, :, None], f"{name}.conv_k.weight": torch.cat([eye, z], 1)[:, :, None],
            f"{name}.conv_v.weight": torch.cat([z, eye], 1)[:, :, None], f"{name}.conv_o.weight": eye[:, :, None]}


def _exact_scale(a):
    """The oracle scales by D^-0.5 in double; the table holds its float32 rounding."""
    return dict(a, qk_scale=a["D"] ** -0.5)


def _oracle_mask(a):
    B, Tq, Tk = a["B"], a["Tq"], a["Tk"]
    m = torch.ones(B, 1, Tq, Tk)
    if a.get("mask_q") is not None:
        m = m * torch.from_numpy(a["mask_q"][:B * Tq].reshape(B, 1, Tq, 1) * a["mask_k"][:B * Tk].reshape(B, 1, 1, Tk))
    if a.get("mask_dense") is not None:
        m = m * torch.from_numpy(R.view(a, "mask_dense", (B, 1, Tq, Tk), (a["mask_dense_bs"], 0, Tk, 1), np.float32))
    return m


ORACLE_MHA = [id for id in R.MHA_IDS if R._BY_ID[id]["B"] * R._BY_ID[id]["Tq"] * R._BY_ID[id]["Tk"] <= 300_000]


@pytest.mark.parametrize("id", ORACLE_MHA)
def test_contract_equals_the_oracle_attention(id):
    """oracle.hsp_oracle.mha_relpos (windowed cases) / mha_plain (the others) with identity 1x1 projections that pick
    q from x and k, v from the two halves of c."""
    from oracle import hsp_oracle as O
    a = _exact_scale(R.args(id))
    B, C, Tq, Tk = a["B"], a["H"] * a["D"], a["Tq"], a["Tk"]
    q, k, v = (t.reshape(B, C, -1) for t in _views(a))
    sd = _sd_identity("att", C)
    mask = _oracle_mask(a) if a.get("mask") else None
    w = R.eff(a)[0]
    if a.get("rel_k") is not None:
        sd["att.emb_rel_k"], sd["att.emb_rel_v"] = _t(a["rel_k"]).view(1, 2 * w + 1, -1), _t(a["rel_v"]).view(1, 2 * w + 1, -1)
        want = O.mha_relpos(sd, "att", q, torch.cat([k, v], 1), mask, a["H"], w)
    else:
        want = O.mha_plain(sd, "att", q, torch.cat([k, v], 1), mask, a["H"])
    got = R.mha_values(a)
    err = np.abs(got - want.numpy()) / np.maximum(1.0, np.abs(want.numpy()))
    assert float(err.max()) <= RTOL, (id, float(err.max()))


@pytest.mark.parametrize("id", ["P_self_t33", "D_self_t33"])
def test_fused_contract_equals_timm_attention_and_mega_mha(id):
    """Both draw q, k and v from ONE input, so the case is read with k = v = q: timm_attention with qkv = three stacked
    identities, mega_mha with identity w_q / w_k / w_v; the output projection is the case's weight and bias."""
    from oracle import hsp_oracle as O
    a = _exact_scale(R.args(id))
    B, C, T, M = a["B"], a["H"] * a["D"], a["Tq"], a["M"]
    q, k, v = (t.reshape(B, C, T) for t in _views(a))
    wt = _t(a["wt"][:M * a["wt_ld"]].reshape(M, a["wt_ld"])[:, :C])
    bias = _t(a["bias"][:M])
    same = dict(a, k=a["q"], v=a["q"], **{f"{n}_{f}": a["q_" + f] for n in "kv" for f in ("off", "bs", "cs")})
    got = R.proj_values(same)
    eye = torch.eye(C, dtype=torch.float64)
    # timm packs qkv as (3, heads, hd) on the feature axis
    sd = {"a.qkv.weight": torch.cat([eye, eye, eye]), "a.proj.weight": wt, "a.proj.bias": bias}
    want = O.timm_attention(sd, "a", q.transpose(1, 2), a["H"]).transpose(1, 2).numpy()
    assert float((np.abs(got - want) / np.maximum(1.0, np.abs(want))).max()) <= RTOL
    sd = {"m.w_q.weight": eye, "m.w_k.weight": eye, "m.w_v.weight": eye, "m.out_proj.0.weight": wt, "m.out_proj.0.bias": bias}
    sd.update({f"m.w_{n}.bias": torch.zeros(C, dtype=torch.float64) for n in "qkv"})
    want = O.mega_mha(sd, "m", q.transpose(1, 2), a["H"]).transpose(1, 2).numpy()
    assert float((np.abs(got - want) / np.maximum(1.0, np.abs(want))).max()) <= RTOL


# ------------------------------------------------------------------------------------------------ plans and coverage
def _plan(L, a, **change):
    s = R.to_struct(a, R.fake_base())
    for k, v in change.items():
        setattr(s, k, v)
    out = (ctypes.c_int32 * 4)()
    rc = L.lib().hsp_mha_plan(ctypes.byref(s), out)
    return rc, tuple(out)


@pytest.mark.parametrize("id", R.MHA_IDS)
def test_mha_case_takes_the_kernel_its_id_names(id, L):
    a = R.args(id)
    rc, (kern, ndb, lds, blocks) = _plan(L, a)
    assert rc == 0, (id, rc)
    assert (kern, ndb) == R.named_kernel(id), (id, R.KERNEL_NAMES[kern], ndb)
    assert 0 < lds <= 160 * 1024, (id, lds)
    qt = 16 if kern in (R.ROW, R.RSTR) else 32
    assert blocks == -(-a["Tq"] // qt) * a["H"] * a["B"], (id, blocks)
    forced = R.eff(a)[1]
    assert forced == ("natural" not in id and kern in (R.MSTR, R.RSTR)), id


# out4 = (kernel, NDB, LDS bytes, workgroups) of one case per reachable (kernel, NDB) pair, written down as numbers from
# the library as it stood before the LDS sizes of mha_decide moved into the kernels' layout functions: a change to those
# functions, to a pitch or to a threshold shows here.
PINNED_PLANS = {
    "TOK1_d20_tq1_tk4_contig": (0, 1, 8448, 6),
    "TOK2_d33_tq16_tk7_side1": (0, 2, 12544, 6),
    "TOK3_d69_tq31_tk9_ocs": (0, 3, 16640, 6),
    "WHOLE1_d20_tq17_tk1_contig_nomask": (1, 1, 20736, 6),
    "WHOLE2_d33_tq15_tk2_side1_factor": (1, 2, 33152, 6),
    "WHOLE3_d69_tq16_tk3_side4_nomask": (1, 3, 45568, 6),
    "WHOLE4_d97_tq31_tk63_own_nomask": (1, 4, 62080, 6),
    "SLAB1_d32_tq300_tk270_side1": (2, 1, 53504, 260),
    "SLAB2_d64_tq300_tk270_contig": (2, 2, 65920, 260),
    "SLAB3_d69_tq33_tk300_side4_causal": (2, 3, 82432, 8),
    "SLAB4_d128_tq33_tk300_contig": (2, 4, 94848, 4),
    "MSTR1_d20_tq17_tk127_contig_nomask": (3, 1, 37504, 4),
    "MSTR2_d64_tq33_tk128_side1_factor": (3, 2, 58112, 8),
    "MSTR3_d69_tq31_tk129_side4_causal": (3, 3, 78720, 4),
    "MSTR4_d128_tq33_tk257_own_factor+irreg": (3, 4, 99328, 8),
    "ROW1_d20_t17_w4_contig_factor": (4, 1, 7808, 8),
    "ROW2_d129_t16_w2_side4_causal": (4, 2, 42368, 4),
    "RSTR1_d20_t255_w4_contig_factor": (5, 1, 23296, 64),
    "RSTR2_d160_t257_w3_side4_causal": (5, 2, 59904, 68),
}


def test_plan_is_pinned(L):
    assert {R.named_kernel(id) for id in PINNED_PLANS} == {(p[0], p[1]) for p in PINNED_PLANS.values()} and len(PINNED_PLANS) == 19
    for id, want in PINNED_PLANS.items():
        rc, got = _plan(L, R.args(id))
        assert rc == 0 and got == want, (id, rc, got, want)


def _reachable(L):
    """Every (kernel, NDB) hsp_mha_plan returns over a sweep of the quantities the decision reads: head dim, key
    count, masks, window, the force-stream hook and the workgroup count."""
    fb = R.fake_base()
    s = R.to_struct(R.args("WHOLE4_d128_tq32_tk64_ocs_factor"), fb)
    out = (ctypes.c_int32 * 4)()
    seen = set()
    for D, Tk, masked, w, force, big in itertools.product(range(1, 257), (1, 4, 100, 256, 257, 300, 900, 2000, 5000),
                                                          (False, True), (0, 4), (False, True), (False, True)):
        s.D, s.Tk, s.Tq = D, Tk, Tk if w else 40
        s.q_cs = s.o_cs = s.k_cs = s.v_cs = 0
        s.B, s.H = (40, 8) if big else (1, 2)
        s.mask_q, s.mask_k = (fb["mask_q"], fb["mask_k"]) if masked else (None, None)
        s.rel_k, s.rel_v = (fb["rel_k"], fb["rel_v"]) if w else (None, None)
        s.window = -(w + 1) if force else w
        assert L.lib().hsp_mha_plan(ctypes.byref(s), out) == 0, (D, Tk, masked, w, force, big)
        seen.add((out[0], out[1]))
    return seen


def test_table_covers_every_kernel_ndb_layout_and_mask_kind(L):
    cases = [R.args(id) for id in R.MHA_IDS]
    named = {R.named_kernel(a["id"]) for a in cases}
    reach = _reachable(L)
    assert reach == {(R.TOK, n) for n in (1, 2, 3)} | {(k, n) for k in (R.WHOLE, R.SLAB, R.MSTR) for n in (1, 2, 3, 4)} | \
        {(k, n) for k in (R.ROW, R.RSTR) for n in (1, 2)}, sorted(reach)
    assert named == reach, ("missing", sorted(reach - named), "unreachable", sorted(named - reach))
    print("covered (kernel, NDB):", ", ".join("%s%d" % (R.KERNEL_NAMES[k], n) for k, n in sorted(named)))
    for kern in range(6):
        mine = [a for a in cases if R.named_kernel(a["id"])[0] == kern]
        lays = {a["layout"] for a in mine}
        assert "contig" in lays and lays & {"side4", "side1"} and {"own", "ocs"} <= lays, (R.KERNEL_NAMES[kern], lays)
        assert {"side4", "side1"} <= lays, (R.KERNEL_NAMES[kern], lays)
        assert {a["reg"] for a in mine} == {"ctl"} | set(R.REGS), R.KERNEL_NAMES[kern]
        assert any(a["Tq"] != a["Tk"] for a in mine if a.get("rel_k") is None), R.KERNEL_NAMES[kern]
        if kern in R.MASKED_CAPABLE:
            kinds = {(a.get("mask_q") is not None, a.get("mask_dense") is not None) for a in mine}
            assert kinds == {(False, False), (True, False), (False, True), (True, True)}, (R.KERNEL_NAMES[kern], kinds)
            assert any("nonbin" in a["mask"] for a in mine), R.KERNEL_NAMES[kern]
            assert any("gap" in a["mask"] for a in mine), R.KERNEL_NAMES[kern]
    for kern in (R.WHOLE, R.MSTR, R.ROW, R.RSTR):                   # fewer keys than one 16-B window
        assert {a["Tk"] for a in cases if R.named_kernel(a["id"])[0] == kern} & {1, 2, 3}, R.KERNEL_NAMES[kern]
    assert {a["D"] for a in cases if R.named_kernel(a["id"])[0] in (R.ROW, R.RSTR) and a.get("rel_k") is None} >= {129, 256}
    pj = [R.args(id) for id in R.PROJ_IDS]
    for cfg in R.PROJ_CFG.values():
        mine = [a for a in pj if (a["H"], a["D"]) == cfg]
        assert {a["Tq"] for a in mine} >= {1, 15, 16, 17, 33}
        assert {a["Tk"] for a in mine} >= {4, 5, 63, 64, 65, 128, 255, 256, 257, 515}
        kl = set(itertools.chain.from_iterable(a["key_len"].tolist() for a in mine if a.get("key_len") is not None))
        assert kl >= {-3, 0, 1, 3, 63, 64, 65, 70, 79}
        assert {a["form"] for a in mine} == {"bmt", "btm", "gen", "last"} and any(a.get("res_is_y") for a in mine)
        assert {a["reg"] for a in mine if a.get("key_len") is None} | {a["reg"] for a in mine if a.get("key_len") is not None} \
            == {"ctl", "stairup100"} | set(R.REGS)
        assert {a["layout"] for a in mine} >= {"contig", "side4", "side1", "dit", "own"}
        assert any(a["wt_ld"] == a["M"] + 4 and a["mask_bs"] == a["Tq"] + 3 and a["cscale_bs"] == a["M"] + 1 for a in mine)
    opts = {tuple(a.get(n) is not None for n in ("bias", "mask", "cscale", "res")) for a in pj}
    assert opts >= {(False, True, True, True), (True, False, True, True), (True, True, False, True),
                    (True, True, True, False), (False, False, False, False), (True, True, True, True)}


# ------------------------------------------------------------------------------------------------ refusals
def test_mha_refusals(L):
    """Each refused struct breaks ONE rule of the decision function; the nearest struct on the allowed side is accepted.
    hsp_mha_f32 launches exactly what hsp_mha_plan accepts (one decision function), so the plan is asked."""
    fb = R.fake_base()
    a = R.args("WHOLE4_d128_tq32_tk64_ocs_factor")
    Tq, Tk = a["Tq"], a["Tk"]
    assert _plan(L, a)[0] == 0 and a["mask_q"] is not None and a["o_cs"] > Tq and (Tq, Tk) == (32, 64)
    for change in (dict(mask_q=None), dict(mask_k=None), dict(q_cs=Tq - 1), dict(k_cs=Tk - 1), dict(v_cs=Tk - 1),
                   dict(o_cs=Tq - 1), dict(q=None), dict(o=None), dict(B=0), dict(D=0), dict(Tk=0),
                   dict(rel_k=fb["rel_k"], rel_v=fb["rel_v"], window=4),            # a window with Tq != Tk
                   dict(mask_dense=fb["mask_dense"], mask_dense_bs=Tq * Tk - 1),
                   dict(D=257)):
        assert _plan(L, a, **change)[0] == L.EINVAL, change
    for change in (dict(mask_q=None, mask_k=None), dict(q_cs=Tq), dict(k_cs=Tk), dict(v_cs=Tk), dict(o_cs=Tq),
                   dict(q_cs=0, k_cs=0, v_cs=0, o_cs=0),
                   dict(mask_dense=fb["mask_dense"], mask_dense_bs=Tq * Tk), dict(D=256)):
        assert _plan(L, a, **change)[0] == 0, change
    w = R.args("ROW1_d64_t33_w4_side1_nomask")
    assert _plan(L, w)[0] == 0 and w["window"] == 4 and w["Tq"] == w["Tk"]
    for change in (dict(window=0), dict(rel_v=None, window=0), dict(Tq=w["Tq"] - 1, q_cs=0, o_cs=0)):
        assert _plan(L, w, **change)[0] == L.EINVAL, change
    assert _plan(L, w, rel_k=None, rel_v=None, window=0)[0] == 0
    # the head-dim limit holds on every path: whole-row and key-streaming, windowed and not, short and long
    for base, extra in ((w, {}), (w, dict(window=-5)), (a, dict(mask_q=None, mask_k=None)), (a, dict(window=-1)),
                        (a, dict(Tk=100000, k_cs=0, v_cs=0))):
        rc256, plan = _plan(L, base, D=256, **extra)
        assert rc256 == 0 and plan[0] in (R.ROW, R.RSTR), (extra, plan)
        assert _plan(L, base, D=257, **extra)[0] == L.EINVAL, extra
    assert L.lib().hsp_mha_plan(None, (ctypes.c_int32 * 4)()) == L.EINVAL


def _proj_refused(L, a, **change):
    """hsp_mha_proj_f32 has no plan form, so this calls the LAUNCHING entry point on made-up addresses and a null
    stream: only a struct that one of the checks in front of the launch refuses may come here (never call it expecting
    0).  The accepted neighbours of these rules -- wt_ld = M + 4, y_ts = 3 and M, Tk = 4 -- are launched for real by
    tests/test_gpu_attn_contract.py."""
    s = R.to_struct(a, R.fake_base())
    for k, v in change.items():
        setattr(s, k, v)
    return L.lib().hsp_mha_proj_f32(ctypes.byref(s), None) == L.EINVAL


def test_mha_proj_refusals(L):
    sup = L.lib().hsp_mha_proj_supported
    assert sup(4, 69, 276, 4) == 1 and sup(4, 69, 276, 3) == 0 and sup(2, 96, 192, 4) == 1 and sup(2, 96, 192, 3) == 0
    assert sup(4, 69, 272, 64) == 0 and sup(2, 96, 196, 64) == 0 and sup(4, 96, 384, 64) == 0 and sup(2, 69, 138, 64) == 0
    assert sup(4, 69, 276, 1 << 20) == 1 and sup(4, 69, 276, (1 << 20) + 1) == 0
    for id in ("P_wide_strides", "D_wide_strides"):
        a = R.args(id)
        M, Tk = a["M"], a["Tk"]
        assert a["wt_ld"] == M + 4 and a["y_ts"] == 3 and a["res"] is not None
        for change in (dict(Tk=3), dict(M=M - 4), dict(wt_ld=M + 2), dict(wt_ld=M + 6), dict(wt_ld=M - 4), dict(y_ts=0),
                       dict(y_ts=-1), dict(res_ts=0), dict(debug=1), dict(k_cs=Tk - 1), dict(v_cs=Tk - 1), dict(q_cs=0),
                       dict(q=None), dict(wt=None), dict(y=None), dict(B=0), dict(Tq=0),
                       # 32-bit offsets inside one utterance's planes: C * stride, M * wt_ld ... must stay below 2^31
                       dict(k_cs=-(-(1 << 31) // M)), dict(v_cs=-(-(1 << 31) // M)), dict(q_cs=-(-(1 << 31) // M)),
                       dict(y_cs=-(-(1 << 31) // M)), dict(res_cs=-(-(1 << 31) // M))):
            assert _proj_refused(L, a, **change), (id, change)


# ------------------------------------------------------------------------------------------------ the two bars
_WORST = {}


def _ratios(id):
    if id not in _WORST:
        a, ref, written = R.case(id)
        got, _ = R.contract(a, np.float32)
        bound = R.derived_bound(a)
        err = np.abs(got - ref)[written]
        assert np.isfinite(got[written]).all(), id
        # (an element the mask zeroes has bound 0 and error 0)
        _WORST[id] = (float((err / np.maximum(bound[written], 1e-300) * (err > 0)).max()), float(err.max()) / H.tol_for(ref[written]),
                      float(bound[written].max()) / max(1.0, float(np.abs(ref[written]).max())))
    return _WORST[id]


@pytest.mark.parametrize("id", R.IDS)
def test_float32_evaluation_lies_within_both_bars(id):
    """The admission condition: the contract evaluated in float32 by numpy (plain order) is within the derived bound,
    element by element, and within the project bar.  A case that is not would be reshaped, never given a wider bar."""
    r_bound, r_bar, rel = _ratios(id)
    assert r_bound <= 1.0 and r_bar <= 1.0, f"{id}: float32 evaluation at {r_bound:.3f} of the derived bound, {r_bar:.3f} of the bar"
    # the bound is a bound on rounding, not a licence: a few per cent of the output's scale at the most (the fused
    # form at 515 keys and a 240-wide staircase reaches 1.6e-2), so no wrong weight of order 0.1 hides under it
    assert rel <= 5e-2, (id, rel)


def test_report_worst_float32_ratios():
    for ent, ids in (("hsp_mha_f32", R.MHA_IDS), ("hsp_mha_proj_f32", R.PROJ_IDS)):
        wb = max(ids, key=lambda i: _ratios(i)[0])
        wp = max(ids, key=lambda i: _ratios(i)[1])
        print(f"float32 numpy vs float64, {ent}: worst derived-bound ratio {_ratios(wb)[0]:.3f} ({wb}), "
              f"worst project-bar ratio {_ratios(wp)[1]:.3f} ({wp})")
