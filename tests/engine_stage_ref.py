"""The stages of the two encoders in fp64, each with a per-element bound: what tests/test_engine_stages_gpu.py holds the executors of
prcv2025reid_amd/engine.py to, stage by stage, on the executor's own saved inputs (checked on its own, against the oracle's whole
encoders and autograd through them, by tests/test_engine_stage_ref_cpu.py).  Device-agnostic torch.

Every stage is the reference model's definition of it: the oracle's functions (layer_norm, mer_linear, linear, attention_core, gelu_erf,
quick_gelu, patch_embed) on a state dict addressed by reference key names.  The backward stages are the hand-written transposes of the
same functions; the CPU file ties them to autograd.

Operands (``Operands``).  ``fmt`` None: the fp64 state dict itself, no rounding anywhere (composition against the oracle).  Otherwise the
16-bit operands an executor holds: per modality a state dict whose shared weights are the merged W + (alpha/r) B_mu A_mu in 16 bits (and
whose lora_B is zero, so that mer_linear adds nothing twice), and the 16-bit adapters for T / U / dA / dB.  ``from_engine`` takes them
from the engine's own packs (the GPU file checks those against the state dict first), ``from_state`` rounds them itself.

Bounds, u = 2^-24, derived from operation counts and never from a run:
  * GEMM with fp32 accumulation over K terms (16-bit x 16-bit products are exact in fp32): (K + 8) u sum|a||b| (bias, epilogue and the
    order of the sum included: a sum of K terms in ANY order, fp32 atomics too, moves by at most (K - 1) u sum|term| to first order),
    plus one rounding of the output format;
  * LayerNorm, its backward, attention and the transcendental epilogues: the references and allowances that the kernel tests already
    state (rowops_refs.ln_stats_ref / ln_y_ref, test_kernels_gpu._ln_bwd_ref / _attn_ref64, helpers.f_gelu ...), imported, plus the
    input error of a transcendental times its Lipschitz constant (|gelu'| <= 1.13, |gelu''| <= 0.8, |quick'| <= 1.1);
  * a value stored in 16 bits: test_kernels_gpu._rounding of (|reference| + allowance).
A bound of exactly 0 (masked, pruned or dropped quantities) demands equality."""
import math

import torch

from oracle import reid_oracle as O
from helpers import f_dgelu, f_gelu, f_quick, round16
from rowops_refs import im2col_ref, ln_stats_ref
from test_kernels_gpu import _attn_ref64, _ln_bwd_ref, _rounding

U32 = 2.0 ** -24
FMT = {'bf16': (7, -126), 'f16': (10, -14), None: (52, -1022)}     # stored mantissa bits, least normal exponent (as _rounding takes them)
LIP_GELU, LIP_DGELU, LIP_QUICK = 1.13, 0.8, 1.1
VIS = 'clip_encoder.vision_layers.'
TXT = 'clip_encoder.clip_model.text_model.'
PROJ = {'qkv': ('attn.q_proj', 'attn.k_proj', 'attn.v_proj'), 'out': ('attn.out_proj',), 'fc1': ('mlp.fc1',), 'fc2': ('mlp.fc2',)}


def rb(v, fmt):
    """Largest error of storing |v| in ``fmt`` ('bf16', 'f16'; 'f32': one fp32 rounding; None: nothing)."""
    if fmt is None:
        return torch.zeros_like(v)
    if fmt == 'f32':
        return U32 * v.abs()
    return _rounding(v, *FMT[fmt])


def ratio(got, ref, bound):
    """Worst |got - ref| / bound over the elements; an error where the bound is 0 gives inf, NaN in ``got`` gives inf.  Elements whose
    bound is inf are not the stage's to write (rows a pruned call leaves out) and are skipped."""
    assert got.shape == ref.shape, (got.shape, ref.shape)
    err = (got.double() - ref).abs()
    bound = torch.as_tensor(bound, dtype=torch.float64, device=err.device).expand_as(err)
    r = torch.where(err == 0, torch.zeros_like(err), err / bound)
    r = torch.where(torch.isnan(r), torch.full_like(r, float('inf')), r)
    r = torch.where(torch.isinf(bound), torch.zeros_like(r), r)
    return float(r.max()) if r.numel() else 0.0


def mer_linear_T(dy, state, prefix, modality, scaling):
    """Transpose of O.mer_linear in its input: dX = dY W + ((dY B) A) (alpha / r)."""
    a = state[f'{prefix}.loras.{modality}.lora_A.weight']
    bm = state[f'{prefix}.loras.{modality}.lora_B.weight']
    return dy @ state[prefix + '.shared_linear.weight'] + ((dy @ bm) @ a) * scaling


def _abs(view):
    return {k: v.abs() for k, v in view.items() if v.is_floating_point()}


class Operands:
    """fwd[m] / bwd[m]: the state dict mer_linear / mer_linear_T read for an image of modality m; plain: the adapters (and everything
    that is no MERLinear weight)."""

    def __init__(self, fwd, bwd, plain):
        self.fwd, self.bwd, self.plain = fwd, bwd, plain
        self._abs = {}

    def mag(self, back, m):
        key = (back, m)
        if key not in self._abs:
            self._abs[key] = _abs((self.bwd if back else self.fwd)[m])
        return self._abs[key]

    @staticmethod
    def exact(state64, vmods):
        return Operands({m: state64 for m in vmods}, {m: state64 for m in vmods}, state64)

    @staticmethod
    def _views(state64, vmods, fmt, merged):
        """``merged(prefix, m, transposed)`` -> fp64 [n_out, K] merged 16-bit weight of one reference MERLinear."""
        plain = dict(state64)
        for k, v in state64.items():
            if '.loras.' in k or k == 'clip_encoder.vision_proj.weight' or (k.startswith('clip_encoder.patch_embeds.') and k.endswith('.weight')):
                plain[k] = round16(v, fmt)                   # every other matrix an MFMA reads: adapters, projection, patch convolutions
        fwd, bwd = {}, {}
        prefixes = [k[:-len('.shared_linear.weight')] for k in state64 if k.endswith('.shared_linear.weight')]
        for m in vmods:
            for views, tr in ((fwd, False), (bwd, True)):
                v = dict(plain)
                for p in prefixes:
                    v[p + '.shared_linear.weight'] = merged(p, m, tr)
                    kb = f'{p}.loras.{m}.lora_B.weight'
                    v[kb] = torch.zeros_like(plain[kb])
                views[m] = v
        return Operands(fwd, bwd, plain)

    @staticmethod
    def from_state(state64, arch, fmt):
        """What an executor would hold, rounded here: merged weights round16(W + (alpha/r) B A)."""
        vmods = [m for m in arch['modalities'] if m != 'text']
        s = arch['lora_alpha'] / arch['lora_rank']
        return Operands._views(state64, vmods, fmt, lambda p, m, tr: round16(
            state64[p + '.shared_linear.weight'] + s * state64[f'{p}.loras.{m}.lora_B.weight'] @ state64[f'{p}.loras.{m}.lora_A.weight'], fmt))

    @staticmethod
    def from_engine(engine, state64):
        """The upcast of the engine's own merged stacks (LoraLayout consulted only to locate each reference linear's slot)."""
        from prcv2025reid_amd.engine import REF_LIN
        lay = engine.lay

        def merged(p, m, tr):
            parts = p.split('.')
            l, (nm, g) = int(parts[2]), REF_LIN[parts[3] + '.' + parts[4]]
            e = lay.ent[(l, nm)]
            n = e['N'] // e['G']
            mu = lay.vmods.index(m)
            if tr:
                return lay.weff(engine._weff, l, nm, transposed=True)[mu][:, g * n:(g + 1) * n].t().double()
            return lay.weff(engine._weff, l, nm)[mu][g * n:(g + 1) * n].double()
        return Operands._views(state64, lay.vmods, engine.flavor, merged)


def ln_stage(x, w, b, fmt):
    """h = O.layer_norm(x) in ``fmt`` with the fp32 statistics: {'h','mean','rstd'} -> (reference, bound).  h's bound carries what the
    statistics' own allowance moves it by, then ln_y_ref's count (4u |t| + u |y|) and the store."""
    mu, dm, rstd, drstd = ln_stats_ref(x, O.LN_EPS)
    y = O.layer_norm(x, w, b)
    t = (y - b).abs()
    cen = (x - mu[:, None]).abs()
    e = w.abs() * (dm[:, None] * rstd[:, None] + cen * drstd[:, None]) + 4 * U32 * t + U32 * y.abs()
    return dict(h=(y, e + rb(y.abs() + e, fmt)), mean=(mu, dm + U32 * mu.abs()), rstd=(rstd, drstd))


class Tower:
    """Stage functions shared by the two towers; a subclass supplies ``_lin`` (one linear on a row set) and the activation."""

    def _gb(self, K, mag):
        return (K + 8) * U32 * mag

    def _heads(self, t, n, S):
        return t.reshape(n, S, self.heads, 64).transpose(1, 2)

    def qkv(self, l, h):
        ys, es = zip(*(self._lin(l, p, h, self.S) for p in PROJ['qkv']))
        y, e = torch.cat(ys, 1), torch.cat(es, 1)
        return y, e + rb(y.abs() + e, self.fmt)

    def allowed(self):
        return torch.ones(1, 1, self.S, self.S, dtype=torch.bool, device=self.dev)

    def _qkv_heads(self, qkv):
        n, S, d = self.n, self.S, self.d
        return [self._heads(qkv[:, i * d:(i + 1) * d], n, S) for i in range(3)]

    def attn(self, qkv, q_rows=None):
        """{'o' [n S, d], 'lse' [n, heads, S]} -> (reference, bound); rows >= q_rows (the pruned last block) are not the call's: their
        bound is inf."""
        n, S, d = self.n, self.S, self.d
        q, k, v = self._qkv_heads(qkv)
        al = self.allowed()
        mask = torch.zeros(al.shape, dtype=torch.float64, device=self.dev).masked_fill(~al, float('-inf'))
        o = O.attention_core(qkv[:, :d].reshape(n, S, d), qkv[:, d:2 * d].reshape(n, S, d), qkv[:, 2 * d:].reshape(n, S, d), self.heads, mask)
        r, b = _attn_ref64(q, k, v, torch.zeros_like(q), al, S, *FMT[self.fmt])
        bo = b['O'] + rb(r['O'].abs() + b['O'], self.fmt)
        bl = b['lse'].clone()
        if q_rows is not None and q_rows < S:
            bo[:, :, q_rows:] = float('inf'); bl[:, :, q_rows:] = float('inf')
        return dict(o=(o.reshape(n * S, d), bo.transpose(1, 2).reshape(n * S, d)), lse=(r['lse'], bl), o_heads=r['O'])

    def attn_bwd(self, qkv, o_saved, do, q_rows=None):
        """{'dqkv' [n S, 3d], 'delta' [n, heads, S]}: delta from the executor's own saved o (a 64-term fp32 sum), dQ / dK / dV from the
        fp64 attention of qkv; dQ of the rows >= q_rows must be exactly 0 and their delta is not published."""
        n, S, d = self.n, self.S, self.d
        q_rows = S if q_rows is None else q_rows
        q, k, v = self._qkv_heads(qkv)
        doh = self._heads(do, n, S)
        r, b = _attn_ref64(q, k, v, doh, self.allowed(), q_rows, *FMT[self.fmt])
        refs, bnds = [], []
        for nm in ('dQ', 'dK', 'dV'):
            rr, bb = r[nm], b[nm]
            bb = bb + rb(rr.abs() + bb, self.fmt)
            if nm == 'dQ':
                rr = rr.clone(); rr[:, :, q_rows:] = 0.0
                bb[:, :, q_rows:] = 0.0
            refs.append(rr.transpose(1, 2).reshape(n * S, d)); bnds.append(bb.transpose(1, 2).reshape(n * S, d))
        prod = doh * self._heads(o_saved, n, S)
        bd = 64 * 2 * U32 * prod.abs().sum(-1) + 2.0 ** -126
        bd[:, :, q_rows:] = float('inf')
        return dict(dqkv=(torch.cat(refs, 1), torch.cat(bnds, 1)), delta=(prod.sum(-1), bd))

    def residual(self, l, nm, x, a, scale, fused):
        """x + scale[image] * (a W^T + b): the branch stored in IEEE half by the blocks that add inside the LayerNorm kernel (``fused``),
        unrounded where the GEMM epilogue adds (the pruned last vision block, the text tower)."""
        rpi = x.shape[0] // self.n
        br, e = self._lin(l, PROJ[nm][0], a, rpi)
        if fused and self.fmt is not None:
            e = e + rb(br.abs() + e, 'f16')
        s = 1.0 if scale is None else scale.repeat_interleave(rpi)[:, None]
        y = x + s * br
        return y, s * e + U32 * (s * br).abs() + 2 * U32 * y.abs()

    def fc1(self, l, h2):
        """{'g', 'u'}: the activation and what the executor saves beside it (vision: gelu'(pre); text: the pre-activation)."""
        rpi = h2.shape[0] // self.n
        pre, e = self._lin(l, PROJ['fc1'][0], h2, rpi)
        return self._act(pre, e)

    def ln_bwd(self, dy, x, w, mean, rstd, dres, bscale, rpi, dx_fmt):
        """{'dx', 'dxb'}: LayerNorm backward from the executor's own statistics plus the residual-stream gradient ``dres``, stored in
        ``dx_fmt``, and its 16-bit copy times the per-image factor ``bscale`` (what enters the next residual branch)."""
        rows = torch.arange(x.shape[0], device=x.device)
        o, allow, _ = _ln_bwd_ref(dy, x, rows, w, mean, rstd, dres)
        bs = 1.0 if bscale is None else bscale.repeat_interleave(rpi)[:, None]
        ob = bs * o
        allow_b = bs * allow + U32 * ob.abs()
        live = 1.0 if bscale is None else (bs != 0).double()    # the copy of an image whose next branch is dropped: exactly 0
        return dict(dx=(o, allow + rb(o.abs() + allow, dx_fmt)), dxb=(ob, allow_b + rb(ob.abs() + allow_b, self.fmt) * live))


class VisionRef(Tower):
    """Vision tower stages for ``mods`` (modality NAME per packed image) and ``drop`` (per layer (s_attn, s_mlp): fp64 [n_img] or None)."""

    def __init__(self, arch, operands, mods, drop, fmt, dx_fmt=None):
        self.a, self.ops, self.mods, self.fmt = arch, operands, list(mods), fmt
        self.dx_fmt = dx_fmt if fmt is not None else None
        self.n = len(self.mods)
        self.L, self.heads, self.d, self.ff = arch['vision_layers'], arch['vision_heads'], arch['vision_hidden_dim'], arch['vision_mlp_dim']
        self.S = (arch['image_size'] // arch['patch_size']) ** 2 + 1
        self.r = arch['lora_rank']
        self.scaling = arch['lora_alpha'] / arch['lora_rank']
        self.vmods = [m for m in arch['modalities'] if m != 'text']
        self.Rp = (len(self.vmods) * self.r + 31) // 32 * 32
        self.drop = drop if drop is not None else [(None, None)] * self.L
        self.dev = operands.plain['clip_encoder.cls_token'].device
        self.q_rows = min(self.S, 32)                         # what q_tiles = 1 keeps in the last block

    def runs(self):
        out, i = [], 0
        while i < self.n:
            j = i
            while j < self.n and self.mods[j] == self.mods[i]:
                j += 1
            out.append((i, j, self.mods[i])); i = j
        return out

    def _lin(self, l, proj, x, rpi, back=False):
        p = f'{VIS}{l}.{proj}'
        fn = mer_linear_T if back else O.mer_linear
        ys, ms = [], []
        for i0, i1, m in self.runs():
            xs = x[i0 * rpi:i1 * rpi]
            ys.append(fn(xs, (self.ops.bwd if back else self.ops.fwd)[m], p, m, self.scaling))
            ms.append(fn(xs.abs(), self.ops.mag(back, m), p, m, self.scaling))
        return torch.cat(ys), self._gb(x.shape[1], torch.cat(ms))

    def _act(self, pre, e):
        _, eg = f_gelu(pre, True)
        du, ed = f_dgelu(pre, True)
        g = O.gelu_erf(pre)
        eg = LIP_GELU * e + eg; ed = LIP_DGELU * e + ed
        return dict(g=(g, eg + rb(g.abs() + eg, self.fmt)), u=(du, ed + rb(du.abs() + ed, self.fmt)))

    # ---- forward
    def embed(self, groups):
        """Layer 0's x [n S, d] from ``groups`` [(modality name, images fp64 [n, 3, H, W])]: patch embedding (im2col rows stored in 16
        bits, the 1-channel mean taken in fp32 first), position, class token."""
        P, a = self.ops.plain, self.a
        pos, cls = P['clip_encoder.vision_pos_embed'], P['clip_encoder.cls_token']
        xs, es = [], []
        for m, img in groups:
            w = P[f'clip_encoder.patch_embeds.{m}.proj.weight']
            pe = O.patch_embed(img, P, m, a['patch_size'])
            n = img.shape[0]
            x = torch.cat([cls.expand(n, -1, -1), pe], 1) + pos[None]
            cols = im2col_ref(img, a['patch_size'], w.shape[1]).abs()
            wf = w.reshape(w.shape[0], -1).abs().t()
            mag = cols @ wf + P[f'clip_encoder.patch_embeds.{m}.proj.bias'].abs() + pos[1:].abs().repeat(n, 1)
            e = (rb(cols, self.fmt) + 4 * U32 * cols) @ wf + self._gb(cols.shape[1], mag) if self.fmt is not None else self._gb(cols.shape[1], mag)
            e = torch.cat([2 * U32 * x[:, :1].abs(), e.view(n, self.S - 1, self.d)], 1)
            xs.append(x.reshape(n * self.S, self.d)); es.append(e.reshape(n * self.S, self.d))
        return torch.cat(xs), torch.cat(es)

    def ln(self, l, which, x):
        p = f'{VIS}{l}.ln{which}.'
        return ln_stage(x, self.ops.plain[p + 'weight'], self.ops.plain[p + 'bias'], self.fmt)

    def cls_rows(self, t):
        return t.view(self.n, self.S, -1)[:, 0]

    def xm(self, l, x, o):
        """x + s_attn * out_proj(o); the last block on the class rows of x and o."""
        last = l == self.L - 1
        return self.residual(l, 'out', x, o, self.drop[l][0], fused=not last)

    def xn(self, l, xm, g):
        last = l == self.L - 1
        return self.residual(l, 'fc2', xm, g, self.drop[l][1], fused=not last)

    def _adapter_cols(self, l, nm, X, key, back):
        """mask_modality(X . cat^T) * alpha/r over the G projections of linear ``nm``: T (key 'lora_A', X = the linear's input) or U
        (key 'lora_B', X = its cotangent dY, per projection its own columns)."""
        rpi = X.shape[0] // self.n
        G, r, Rp = len(PROJ[nm]), self.r, self.Rp
        out = torch.zeros(X.shape[0], G * Rp, dtype=torch.float64, device=X.device)
        e = torch.zeros_like(out)
        n_out = X.shape[1] // G
        for i0, i1, m in self.runs():
            mu = self.vmods.index(m)
            for g, proj in enumerate(PROJ[nm]):
                w = self.ops.plain[f'{VIS}{l}.{proj}.loras.{m}.{key}.weight']
                xs = X[i0 * rpi:i1 * rpi]
                if back:
                    xs = xs[:, g * n_out:(g + 1) * n_out]; w = w.t()
                t = xs @ w.t() * self.scaling
                c = slice(g * Rp + mu * r, g * Rp + (mu + 1) * r)
                out[i0 * rpi:i1 * rpi, c] = t
                e[i0 * rpi:i1 * rpi, c] = self._gb(xs.shape[1], xs.abs() @ w.abs().t() * self.scaling) + U32 * t.abs()
        return out, e + rb(out.abs() + e, self.fmt) * (e > 0)

    def T(self, l, nm, X):
        return self._adapter_cols(l, nm, X, 'lora_A', False)

    def head(self, x_final):
        """{'cls_h','mf','rf','feats'} from the class rows leaving the last block."""
        P = self.ops.plain
        s = ln_stage(x_final, P['clip_encoder.vision_ln_final.weight'], P['clip_encoder.vision_ln_final.bias'], self.fmt)
        return dict(cls_h=s['h'], mf=s['mean'], rf=s['rstd'])

    def feats(self, cls_h):
        w = self.ops.plain['clip_encoder.vision_proj.weight']
        y = cls_h @ w.t()
        return y, self._gb(w.shape[1], cls_h.abs() @ w.abs().t()) + U32 * y.abs()

    # ---- backward (scaled domain)
    def dfb(self, dfeat_scaled):
        return dfeat_scaled, rb(dfeat_scaled.abs(), self.fmt)

    def dcls(self, dfb):
        w = self.ops.plain['clip_encoder.vision_proj.weight']
        y = dfb @ w
        e = self._gb(w.shape[0], dfb.abs() @ w.abs())
        return y, e + rb(y.abs() + e, self.fmt)

    def ln_final_bwd(self, dcls, x_final, mf, rf):
        return self.ln_bwd(dcls, x_final, self.ops.plain['clip_encoder.vision_ln_final.weight'], mf, rf, None, self.drop[-1][1], 1, self.dx_fmt)

    def _dx(self, l, nm, dY):
        rpi = dY.shape[0] // self.n
        n_out = dY.shape[1] // len(PROJ[nm])
        ys, es = zip(*(self._lin(l, p, dY[:, g * n_out:(g + 1) * n_out], rpi, back=True) for g, p in enumerate(PROJ[nm])))
        K = dY.shape[1]
        return sum(ys), sum(es) * (K + 8) / (n_out + 8)

    def du(self, l, gyb, u):
        y, e = self._dx(l, 'fc2', gyb)
        y, e = y * u, e * u.abs() + U32 * (y * u).abs()
        return y, e + rb(y.abs() + e, self.fmt)

    def dx_lin(self, l, nm, dY):
        """dh2 = du W1 (nm 'fc1'), do = dxmb Wo ('out'), dh = dqkv Wqkv ('qkv'): the cotangent of a linear's input in 16 bits."""
        y, e = self._dx(l, nm, dY)
        return y, e + rb(y.abs() + e, self.fmt)

    def ln2_bwd(self, l, dh2, xm, mean2, rstd2, gy):
        rpi = xm.shape[0] // self.n
        return self.ln_bwd(dh2, xm, self.ops.plain[f'{VIS}{l}.ln2.weight'], mean2, rstd2, gy, self.drop[l][0], rpi, self.dx_fmt)

    def ln1_bwd(self, l, dh, x, mean1, rstd1, dxm):
        return self.ln_bwd(dh, x, self.ops.plain[f'{VIS}{l}.ln1.weight'], mean1, rstd1, dxm, self.drop[l - 1][1] if l > 0 else None, self.S,
                           self.dx_fmt)

    def scatter(self, rows_t):
        """Class-row tensor [n, c] back to all rows [n S, c]: zero everywhere else, exactly."""
        out = torch.zeros(self.n, self.S, rows_t.shape[1], dtype=torch.float64, device=rows_t.device)
        out[:, 0] = rows_t
        out = out.view(self.n * self.S, -1)
        return out, torch.zeros_like(out)

    def U(self, l, nm, dY):
        return self._adapter_cols(l, nm, dY, 'lora_B', True)

    def adapter_grads(self, l, nm, dY, X, T, U, scale):
        """{reference key: (gradient, bound)} of every adapter tensor of linear ``nm`` of layer ``l``, every modality: dB = dY^T T and
        dA = U^T X over the rows of the modality's images, unscaled; exactly 0 for a modality no image has."""
        rpi = dY.shape[0] // self.n
        G, r, Rp = len(PROJ[nm]), self.r, self.Rp
        n_out = dY.shape[1] // G
        out = {}
        for mu, m in enumerate(self.vmods):
            rows = torch.tensor([i for i in range(self.n) if self.mods[i] == m], dtype=torch.long, device=dY.device)
            rows = (rows[:, None] * rpi + torch.arange(rpi, device=dY.device)[None]).reshape(-1)
            terms = rows.numel()
            for g, proj in enumerate(PROJ[nm]):
                c = slice(g * Rp + mu * r, g * Rp + (mu + 1) * r)
                dYg = dY[rows][:, g * n_out:(g + 1) * n_out]
                for key, a, b in (('lora_B', dYg, T[rows][:, c]), ('lora_A', U[rows][:, c], X[rows])):
                    y = a.t() @ b / scale
                    e = (terms + 8) * U32 * (a.abs().t() @ b.abs()) / scale + U32 * y.abs()
                    out[f'{VIS}{l}.{proj}.loras.{m}.{key}.weight'] = (y, e)
        return out

    def dense_lin(self, l, nm, dY, X, scale):
        """{reference key: (gradient, bound)} of the shared weight and bias of linear ``nm``: dY^T X and the column sums of dY."""
        n_out = dY.shape[1] // len(PROJ[nm])
        M = dY.shape[0]
        out = {}
        for g, proj in enumerate(PROJ[nm]):
            dYg = dY[:, g * n_out:(g + 1) * n_out]
            y = dYg.t() @ X / scale
            out[f'{VIS}{l}.{proj}.shared_linear.weight'] = (y, (M + 8) * U32 * (dYg.abs().t() @ X.abs()) / scale + U32 * y.abs())
            yb = dYg.sum(0) / scale
            out[f'{VIS}{l}.{proj}.shared_linear.bias'] = (yb, (M + 8) * U32 * dYg.abs().sum(0) / scale + U32 * yb.abs())
        return out

    def dense_ln(self, key, dy, x, mean, rstd, scale):
        """(dgamma, dbeta) of a LayerNorm from the executor's own statistics: per column a sum of rows fp32 terms, through atomics."""
        xh = (x - mean[:, None]) * rstd[:, None]
        n = x.shape[0] + 8
        out = {}
        for nm, t in (('weight', dy * xh), ('bias', dy)):
            y = t.sum(0) / scale
            out[f'{key}.{nm}'] = (y, (n * U32 * t.abs().sum(0) + 4 * U32 * t.abs().sum(0)) / scale + U32 * y.abs())
        return out

    def dense_embed(self, dx0, groups, scale):
        """Position and class embeddings and the patch convolutions from dx0 [n S, d], the (scaled) gradient of the embedded sequence:
        the executor sums dx0 over images in fp32 and forms the convolutions' gradients on 16-bit copies of dx0's patch rows and of the
        im2col rows."""
        P, a = self.ops.plain, self.a
        n, S, d = self.n, self.S, self.d
        d3 = dx0.view(n, S, d)
        y = d3.sum(0) / scale
        e = (n + 8) * U32 * d3.abs().sum(0) / scale + U32 * y.abs()
        out = {'clip_encoder.vision_pos_embed': (y, e), 'clip_encoder.cls_token': (y[0].view(1, 1, d), e[0].view(1, 1, d))}
        start = 0
        for m, img in groups:
            w = P[f'clip_encoder.patch_embeds.{m}.proj.weight']
            k = img.shape[0]
            cols = im2col_ref(img, a['patch_size'], w.shape[1])
            dP = d3[start:start + k, 1:].reshape(k * (S - 1), d)
            terms = dP.shape[0]
            gw = dP.t() @ cols / scale
            ca, da = cols.abs(), dP.abs()
            ec, ed = rb(ca, self.fmt) + 4 * U32 * ca, rb(da, self.fmt)
            ew = ((da + ed).t() @ ec + ed.t() @ ca + (terms + 8) * U32 * (da.t() @ ca)) / scale + 2 * U32 * gw.abs()
            gb_ = dP.sum(0) / scale
            eb = (ed.sum(0) + (terms + 8) * U32 * da.sum(0)) / scale + 2 * U32 * gb_.abs()
            kw, kb = f'clip_encoder.patch_embeds.{m}.proj.weight', f'clip_encoder.patch_embeds.{m}.proj.bias'
            for key, y_, e_ in ((kw, gw.view(w.shape), ew.view(w.shape)), (kb, gb_, eb)):
                out[key] = (out[key][0] + y_, out[key][1] + e_) if key in out else (y_, e_)
            start += k
        return out


class TextRef(Tower):
    """Text tower stages: plain linears on 16-bit weights, causal attention with a key mask, quick-GELU, first-EOS pooling."""

    def __init__(self, arch, state, ids, key_mask, fmt):
        self.a, self.P, self.fmt = arch, state, fmt
        self.ids, self.km = ids, key_mask
        self.n, self.S = ids.shape
        self.L, self.heads, self.d, self.ff = arch['text_layers'], arch['text_heads'], arch['text_hidden_dim'], arch['text_mlp_dim']
        self.dev = ids.device

    @staticmethod
    def operands(state64, fmt):
        """The state dict with every matrix an MFMA reads rounded to 16 bits (fmt None: the state dict itself)."""
        if fmt is None:
            return state64
        out = dict(state64)
        for k, v in state64.items():
            if (k.startswith(TXT + 'encoder.layers.') and k.endswith('proj.weight') or k.endswith('.mlp.fc1.weight') and k.startswith(TXT)
                    or k.endswith('.mlp.fc2.weight') and k.startswith(TXT) or k == 'clip_encoder.text_proj.weight'):
                out[k] = round16(v, fmt)
        return out

    def _lin(self, l, proj, x, rpi, back=False):
        proj = proj.replace('attn.', 'self_attn.')
        w, b = self.P[f'{TXT}encoder.layers.{l}.{proj}.weight'], self.P[f'{TXT}encoder.layers.{l}.{proj}.bias']
        return O.linear(x, w, b), self._gb(x.shape[1], O.linear(x.abs(), w.abs(), b.abs()))

    def _act(self, pre, e):
        _, eg = f_quick(pre)
        g = O.quick_gelu(pre)
        eg = LIP_QUICK * e + eg
        return dict(g=(g, eg + rb(g.abs() + eg, self.fmt)), u=(pre, e + rb(pre.abs() + e, self.fmt)))

    def allowed(self):
        T = self.S
        al = torch.ones(1, 1, T, T, dtype=torch.bool, device=self.dev).tril()
        if self.km is not None:
            al = al & self.km.bool().view(self.n, 1, 1, T)
        return al

    def embed(self):
        x = self.P[TXT + 'embeddings.token_embedding.weight'][self.ids] + self.P[TXT + 'embeddings.position_embedding.weight'][:self.S][None]
        x = x.reshape(self.n * self.S, self.d)
        return x, U32 * x.abs()

    def ln(self, l, which, x):
        p = f'{TXT}encoder.layers.{l}.layer_norm{which}.'
        return ln_stage(x, self.P[p + 'weight'], self.P[p + 'bias'], self.fmt)

    def xm(self, l, x, o):
        return self.residual(l, 'out', x, o, None, fused=False)

    def xn(self, l, xm, g):
        return self.residual(l, 'fc2', xm, g, None, fused=False)

    def pool_rows(self):
        eos = (self.ids == self.a['text_eos_id']).int().argmax(dim=-1)
        return torch.arange(self.n, device=self.dev) * self.S + eos

    def head(self, x_final):
        """{'pooled','mf','rf'} of the rows at each sequence's first EOS."""
        s = ln_stage(x_final[self.pool_rows()], self.P[TXT + 'final_layer_norm.weight'], self.P[TXT + 'final_layer_norm.bias'], self.fmt)
        return dict(pooled=s['h'], mf=s['mean'], rf=s['rstd'])

    def feats(self, pooled):
        w = self.P['clip_encoder.text_proj.weight']
        y = pooled @ w.t()
        return y, self._gb(w.shape[1], pooled.abs() @ w.abs().t()) + U32 * y.abs()


# ---------------------------------------------------------------------------------------------------------------- composition
def store(t, fmt):
    """What an executor keeps of a stage output: rounded to ``fmt`` ('bf16' / 'f16'), or as it is (None, 'f32': the fp32 rounding is
    far below every bound and is left out)."""
    return t if fmt in (None, 'f32') else round16(t, fmt)


def vision_forward(ref, groups):
    """The forward stages composed, each output stored in the format the executor stores it in (ref.fmt None: no rounding at all) ->
    (features, state) with the executor's saved-state names."""
    f = ref.fmt
    x, _ = ref.embed(groups)
    layers = []
    for l in range(ref.L):
        last = l == ref.L - 1
        s1 = ref.ln(l, 1, x)
        h = store(s1['h'][0], f)
        qkv = store(ref.qkv(l, h)[0], f)
        at = ref.attn(qkv, ref.q_rows if last else None)
        o = store(at['o'][0], f)
        xin, oin = (ref.cls_rows(x), ref.cls_rows(o)) if last else (x, o)
        xm = ref.xm(l, xin, oin)[0]
        s2 = ref.ln(l, 2, xm)
        h2 = store(s2['h'][0], f)
        a = ref.fc1(l, h2)
        g, u = store(a['g'][0], f), store(a['u'][0], f)
        xn = ref.xn(l, xm, g)[0]
        sa, sm = ref.drop[l]
        layers.append(dict(x=x, h=h, mean1=s1['mean'][0], rstd1=s1['rstd'][0], qkv=qkv, o=o, lse=at['lse'][0], o_rows=oin, xm=xm, h2=h2,
                           mean2=s2['mean'][0], rstd2=s2['rstd'][0], u=u, g=g, sa=sa, sm=sm, cls=last,
                           T=store(ref.T(l, 'qkv', h)[0], f), To=store(ref.T(l, 'out', oin)[0], f), T1=store(ref.T(l, 'fc1', h2)[0], f),
                           T2=store(ref.T(l, 'fc2', g)[0], f)))
        x = xn
    hd = ref.head(x)
    cls_h = store(hd['cls_h'][0], f)
    feats = ref.feats(cls_h)[0]
    return feats, dict(layers=layers, x_final=x, mf=hd['mf'][0], rf=hd['rf'][0], cls_h=cls_h, groups=groups)


def vision_backward(ref, st, dfeat, scale=1.0, want_dense=False):
    """The backward stages composed on a state of ``vision_forward`` -> {reference key: gradient}; every intermediate stored in the
    format the executor stores it in."""
    f, fx = ref.fmt, ref.dx_fmt
    L = ref.L
    grads = {}
    dfb = store(ref.dfb(dfeat * scale)[0], f)
    dcls = store(ref.dcls(dfb)[0], f)
    if want_dense:
        grads['clip_encoder.vision_proj.weight'] = dfb.t() @ st['cls_h'] / scale
        grads.update({k: v[0] for k, v in ref.dense_ln('clip_encoder.vision_ln_final', dcls, st['x_final'], st['mf'], st['rf'], scale).items()})
    b = ref.ln_final_bwd(dcls, st['x_final'], st['mf'], st['rf'])
    gy, gyb = store(b['dx'][0], fx), store(b['dxb'][0], f)
    for l in reversed(range(L)):
        s = st['layers'][l]
        keep = lambda d: grads.update({k: v[0] for k, v in d.items()})
        du = store(ref.du(l, gyb, s['u'])[0], f)
        keep(ref.adapter_grads(l, 'fc2', gyb, s['g'], s['T2'], store(ref.U(l, 'fc2', gyb)[0], f), scale))
        dh2 = store(ref.dx_lin(l, 'fc1', du)[0], f)
        keep(ref.adapter_grads(l, 'fc1', du, s['h2'], s['T1'], store(ref.U(l, 'fc1', du)[0], f), scale))
        b = ref.ln2_bwd(l, dh2, s['xm'], s['mean2'], s['rstd2'], gy)
        dxm, dxmb = store(b['dx'][0], fx), store(b['dxb'][0], f)
        do = store(ref.dx_lin(l, 'out', dxmb)[0], f)
        keep(ref.adapter_grads(l, 'out', dxmb, s['o_rows'], s['To'], store(ref.U(l, 'out', dxmb)[0], f), scale))
        if want_dense:
            keep(ref.dense_lin(l, 'fc2', gyb, s['g'], scale)); keep(ref.dense_lin(l, 'fc1', du, s['h2'], scale))
            keep(ref.dense_lin(l, 'out', dxmb, s['o_rows'], scale))
            keep(ref.dense_ln(f'{VIS}{l}.ln2', dh2, s['xm'], s['mean2'], s['rstd2'], scale))
        if s['cls']:
            do, dxm = ref.scatter(do)[0], ref.scatter(dxm)[0]
        dqkv = store(ref.attn_bwd(s['qkv'], s['o'], do, ref.q_rows if s['cls'] else None)['dqkv'][0], f)
        keep(ref.adapter_grads(l, 'qkv', dqkv, s['h'], s['T'], store(ref.U(l, 'qkv', dqkv)[0], f), scale))
        if l == 0 and not want_dense:
            break
        dh = store(ref.dx_lin(l, 'qkv', dqkv)[0], f)
        if want_dense:
            keep(ref.dense_lin(l, 'qkv', dqkv, s['h'], scale))
            keep(ref.dense_ln(f'{VIS}{l}.ln1', dh, s['x'], s['mean1'], s['rstd1'], scale))
        b = ref.ln1_bwd(l, dh, s['x'], s['mean1'], s['rstd1'], dxm)
        gy, gyb = store(b['dx'][0], fx), store(b['dxb'][0], f)
    if want_dense:
        grads.update({k: v[0] for k, v in ref.dense_embed(gy, st['groups'], scale).items()})
    return grads


def text_forward(ref):
    f = ref.fmt
    x, _ = ref.embed()
    layers = []
    for l in range(ref.L):
        s1 = ref.ln(l, 1, x)
        h = store(s1['h'][0], f)
        qkv = store(ref.qkv(l, h)[0], f)
        at = ref.attn(qkv)
        o = store(at['o'][0], f)
        xm = ref.xm(l, x, o)[0]
        s2 = ref.ln(l, 2, xm)
        h2 = store(s2['h'][0], f)
        a = ref.fc1(l, h2)
        g = store(a['g'][0], f)
        layers.append(dict(x=x, h=h, qkv=qkv, o=o, xm=xm, h2=h2, g=g, u=store(a['u'][0], f)))
        x = ref.xn(l, xm, g)[0]
    hd = ref.head(x)
    return ref.feats(store(hd['pooled'][0], f))[0], dict(layers=layers, x_final=x)
