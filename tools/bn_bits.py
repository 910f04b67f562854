#!/usr/bin/env python3
"""SHA-256 of what the BatchNorm entry points of libfmri_hip.so write (csrc/norm.hip: fmri_bn_*, fmri_act_bwd,
fmri_colsum_rows), one line per case and output.  The inputs are drawn with numpy on the host from fixed seeds, so two
builds of the library that compute the same bits print the same text:

    FMRI_LIB_PATH=/other/checkout/.../libfmri_hip.so python tools/bn_bits.py > old.txt && \\
        python tools/bn_bits.py > new.txt && cmp old.txt new.txt

(one fresh process per build; FMRI_LIB_PATH is read by fmri_hip/lib.py).  The cases are the smallest that reach every
path of the file: the one-launch column kernels, the streaming kernels with one / an idle / several chunk columns, two
block columns and gy > 1, one- and two-stage folds with 1, 2 and 4 groups, and the counting variants on cotangents with
planted overflows, an inf and NaNs.
"""
import hashlib
import os
import sys
import zlib

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "thesis-fmri-reconstruction_amd"))

import torch                    # noqa: E402
from fmri_hip import lib        # noqa: E402

DEV = "cuda:0"
EPS, MOM = 1e-5, 0.9


def P(t):
    return None if t is None else t.data_ptr()


def rng(*key):
    return np.random.default_rng(zlib.crc32(repr(key).encode()))


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def f16(r, shape, scale=1.0, shift=0.0):
    return dev((r.standard_normal(shape) * scale + shift).astype(np.float16))


def f32(r, shape, scale=1.0, shift=0.0):
    return dev((r.standard_normal(shape) * scale + shift).astype(np.float32))


def emit(case, **outs):
    torch.cuda.synchronize()
    for name, t in outs.items():
        print(f"{case} {name} {hashlib.sha256(t.cpu().numpy().tobytes()).hexdigest()}", flush=True)


class Finalize:
    """The finalize arguments of an entry point (fresh outputs, running statistics that are not 0 / 1)."""

    def __init__(self, r, C):
        self.gamma, self.beta = f32(r, C, 0.2, 1.0), f32(r, C, 0.1)
        self.rm, self.rv = f32(r, C, 0.1), dev(np.abs(r.standard_normal(C)).astype(np.float32) + 0.5)
        self.mean, self.rstd, self.scale, self.shift = (torch.zeros(C, device=DEV) for _ in range(4))
        self.nbt = torch.full((), 3, dtype=torch.int64, device=DEV)

    def args(self, updates):
        return (P(self.gamma), P(self.beta), EPS, MOM, updates, P(self.rm), P(self.rv), P(self.mean), P(self.rstd),
                P(self.scale), P(self.shift))

    def outs(self):
        return dict(mean=self.mean, rstd=self.rstd, scale=self.scale, shift=self.shift, running_mean=self.rm,
                    running_var=self.rv, nbt=self.nbt)


def plant(dy):
    """Three finite overflows of dx, one inf and two NaNs: dx = gamma rstd (g - ..) follows a huge / non-finite g."""
    flat = dy.view(-1)
    n = flat.numel()
    for k, v in enumerate((60000.0, -60000.0, 65504.0, float("inf"), float("nan"), float("nan"))):
        flat[(k * 7919 + 13) % n] = v
    return dy


def column_path(M, C):
    r = rng("cols", M, C)
    x = f16(r, (M, C), 1.5, 0.3)
    s = dev(np.array([4.0], np.float32))
    for relu in (0, 1):
        fin = Finalize(r, C)
        y, sums = torch.empty_like(x), torch.zeros(2, C, device=DEV)
        lib.call("fmri_bn_cols_fwd_s", P(x), P(y), M, C, float(M), *fin.args(2), P(sums), P(fin.nbt), relu, P(s))
        emit(f"cols_fwd_s M={M} C={C} relu={relu}", y=y, sums=sums, **fin.outs())
    for ns in (1, 2):
        dy = f16(r, (ns * M, C))
        for pstream in range(ns):
            for relu in (0, 1):
                for counted in (False, True):
                    dx, sums = torch.empty_like(dy), torch.zeros(2 * ns, C, device=DEV)
                    dbeta, dgamma = f32(rng("pg", C), C), f32(rng("pg2", C), C)
                    cnt = torch.zeros(2, dtype=torch.int32, device=DEV)
                    a = (P(x), P(dy), P(dx), M, C, ns, float(M), P(fin.mean), P(fin.rstd), P(fin.gamma), P(fin.beta),
                         relu, P(sums), P(dbeta), P(dgamma), 0.25, pstream)
                    if counted:
                        lib.call("fmri_bn_cols_bwd_cnt", *a, P(cnt))
                    else:
                        lib.call("fmri_bn_cols_bwd", *a)
                    emit(f"cols_bwd{'_cnt' if counted else ''} M={M} C={C} ns={ns} pstream={pstream} relu={relu}",
                         dx=dx, sums=sums, dbeta=dbeta, dgamma=dgamma, cnt=cnt)


def streaming_path(M, C):
    r = rng("stream", M, C)
    L = lib.load()
    tag = f"M={M} C={C}"
    x = f16(r, (M, C), 1.5, 0.3)
    wsf = L.fmri_bn_ws_floats(M, C)
    ws = torch.empty(2 * wsf, device=DEV)
    sums = torch.zeros(2, C, device=DEV)
    lib.call("fmri_bn_stats", P(x), M, C, P(sums), P(ws), wsf)
    emit(f"stats {tag}", sums=sums)
    fin = Finalize(r, C)
    lib.call("fmri_bn_finalize", P(sums), C, float(M), *fin.args(1), P(fin.nbt))
    emit(f"finalize {tag}", **fin.outs())
    fin = Finalize(r, C)
    s = dev(np.array([0.5], np.float32))
    lib.call("fmri_bn_finalize_s", P(sums), C, float(M), *fin.args(2), P(fin.nbt), P(s))
    emit(f"finalize_s {tag}", **fin.outs())
    fin = Finalize(r, C)
    sums = torch.zeros(2, C, device=DEV)
    lib.call("fmri_bn_stats_finalize", P(x), M, C, P(sums), P(ws), wsf, float(M), *fin.args(2), P(fin.nbt))
    emit(f"stats_finalize {tag}", sums=sums, **fin.outs())
    for relu in (0, 1):
        y = torch.empty_like(x)
        lib.call("fmri_bn_apply", P(x), P(y), M, C, P(fin.scale), P(fin.shift), relu)
        emit(f"apply {tag} relu={relu}", y=y)
    stat = (P(fin.mean), P(fin.rstd), P(fin.gamma), P(fin.beta))
    for ns, two in ((1, ""), (2, "2")):
        dy = f16(r, (ns * M, C))
        for relu in (0, 1):
            for pstream in range(ns):
                for grads in (False, True):
                    sums = torch.zeros(2 * ns, C, device=DEV)
                    dbeta, dgamma = f32(rng("pg", C), C), f32(rng("pg2", C), C)
                    lib.call("fmri_bn_bwd_reduce" + two, P(x), P(dy), M, C, *stat, relu, P(sums), P(ws), ns * wsf,
                             P(dbeta) if grads else None, P(dgamma) if grads else None, 0.25, *(pstream,) * (ns - 1))
                    emit(f"bwd_reduce{two} {tag} relu={relu} pstream={pstream} grads={int(grads)}", sums=sums,
                         dbeta=dbeta, dgamma=dgamma)
            for counted in (False, True):
                dx = torch.empty_like(dy)
                cnt = torch.zeros(2, dtype=torch.int32, device=DEV)
                a = (P(x), P(dy), P(dx), M, C, float(M), *stat, relu, P(sums))
                lib.call("fmri_bn_bwd_apply" + two + ("_cnt" if counted else ""), *a, *((P(cnt),) if counted else ()))
                emit(f"bwd_apply{two}{'_cnt' if counted else ''} {tag} relu={relu}", dx=dx, cnt=cnt)


def folds(rows, C):
    r = rng("fold", rows, C)
    L = lib.load()
    tag = f"rows={rows} C={C}"
    scratch = torch.empty(4 * L.fmri_bn_fold_scratch_floats(C), device=DEV)
    part = f32(r, (rows, 2, C), 1.0, 0.5)
    sums = torch.zeros(2, C, device=DEV)
    lib.call("fmri_bn_fold", P(part), rows, C, P(scratch), P(sums))
    emit(f"fold {tag}", sums=sums)
    fin = Finalize(r, C)
    sums = torch.zeros(2, C, device=DEV)
    part[:, 1] = part[:, 1].abs() * 4          # sum x^2 >= (sum x)^2 / n: a variance above zero
    lib.call("fmri_bn_fold_finalize", P(part), rows, C, P(scratch), P(sums), 128.0 * rows, *fin.args(1), P(fin.nbt))
    emit(f"fold_finalize {tag}", sums=sums, **fin.outs())
    for groups in (1, 2, 4):
        cap = rows + 5
        part = f32(r, (groups, cap, 2, C))
        for pgroup in range(groups):
            sums = torch.zeros(groups, 2, C, device=DEV)
            dbeta, dgamma = f32(rng("pg", C), C), f32(rng("pg2", C), C)
            lib.call("fmri_bn_bwd_fold", P(part), rows, cap, C, groups, P(scratch), P(sums), P(dbeta), P(dgamma), 0.25,
                     pgroup)
            emit(f"bwd_fold {tag} groups={groups} pgroup={pgroup}", sums=sums, dbeta=dbeta, dgamma=dgamma)


def act_and_colsum(M, C):
    r = rng("act", M, C)
    L = lib.load()
    y, dy = f16(r, (M, C)), f16(r, (M, C))
    wsf = L.fmri_bn_ws_floats(M, C)
    ws = torch.empty(wsf, device=DEV)
    for act in (0, 1, 2):                   # none, ReLU, tanh
        for bias in (False, True):
            dpre, colsum = torch.empty_like(dy), torch.zeros(2, C, device=DEV)
            dbias = f32(rng("pg", C), C)
            lib.call("fmri_act_bwd", P(y), P(dy), P(dpre), M, C, act, P(colsum), P(ws), wsf,
                     P(dbias) if bias else None, C - 3, 0.5)
            emit(f"act_bwd M={M} C={C} act={act} dbias={int(bias)}", dpre=dpre, colsum=colsum[0], dbias=dbias)
    dpre = torch.empty_like(dy)
    lib.call("fmri_act_bwd", P(y), P(dy), P(dpre), M, C, 1, None, None, 0, None, 0, 0.0)
    emit(f"act_bwd M={M} C={C} act=1 no colsum", dpre=dpre)
    for bias in (False, True):
        sums, dbias = torch.zeros(2, C, device=DEV), f32(rng("pg", C), C)
        lib.call("fmri_colsum_rows", P(y), M, C, P(sums), P(ws), wsf, P(dbias) if bias else None, C - 3, 0.5)
        emit(f"colsum_rows M={M} C={C} dbias={int(bias)}", sums=sums, dbias=dbias)


def counted(M, C):
    """The counting variants on cotangents with planted overflows, no ReLU mask (up to 2048 rows: the column kernel, whose
    own sums take the planted values in).  x has a small variance: rstd ~ 20 carries a cotangent of 60000 past fp16."""
    r = rng("counted", M, C)
    L = lib.load()
    x = f16(r, (M, C), 0.05, 0.3)
    fin = Finalize(r, C)
    wsf = L.fmri_bn_ws_floats(M, C)
    ws = torch.empty(2 * wsf, device=DEV)
    sums = torch.zeros(2, C, device=DEV)
    lib.call("fmri_bn_stats_finalize", P(x), M, C, P(sums), P(ws), wsf, float(M), *fin.args(0), P(fin.nbt))
    stat = (P(fin.mean), P(fin.rstd), P(fin.gamma), P(fin.beta))
    for ns, two in ((1, ""), (2, "2")):
        dy = plant(f16(r, (ns * M, C)))
        dx, cnt = torch.empty_like(dy), torch.zeros(2, dtype=torch.int32, device=DEV)
        sums = torch.zeros(2 * ns, C, device=DEV)
        if M <= 2048:
            lib.call("fmri_bn_cols_bwd_cnt", P(x), P(dy), P(dx), M, C, ns, float(M), *stat, 0, P(sums), None, None, 0.0,
                     0, P(cnt))
        else:
            # sums of the clean cotangent: a NaN in the sums would turn every dx of its channel into NaN
            clean = torch.nan_to_num(dy, 0.0, 0.0, 0.0)
            lib.call("fmri_bn_bwd_reduce" + two, P(x), P(clean), M, C, *stat, 0, P(sums), P(ws), ns * wsf, None, None,
                     0.0, *(0,) * (ns - 1))
            lib.call("fmri_bn_bwd_apply" + two + "_cnt", P(x), P(dy), P(dx), M, C, float(M), *stat, 0, P(sums), P(cnt))
        emit(f"counted M={M} C={C} ns={ns}", dx=dx, saturated=cnt[0], nan=cnt[1])


def main():
    print(f"# {os.path.basename(__file__)}: sha256 of the outputs of the BatchNorm entry points")
    for M, C in ((6, 8), (37, 64), (2048, 72)):
        column_path(M, C)
    for M, C in ((2049, 8), (2049, 64), (4100, 24), (2100, 2056), (70000, 32)):
        streaming_path(M, C)
    for rows in (1, 31, 512, 513, 1500):
        for C in (8, 40):
            folds(rows, C)
    act_and_colsum(2049, 64)
    for M, C in ((2049, 64), (37, 64)):
        counted(M, C)


if __name__ == "__main__":
    main()
