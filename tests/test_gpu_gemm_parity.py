"""Every launch route of the GEMM family (csrc/gemm_f32.hip, gemm_wide.hip, gemm_bf16.hip, gemm_group.hip, gemm_p3.hip, gemm_b1.hip,
gemm_rows.hip, frame_dx.hip) against the fp64 restatement of the operation, tile by tile: one parametrised test per route, named after
the kernel variant sdumc_profile_report gives the launch.  Runs, references, slicing and bars: tests/gemm_cases.py; what makes the bars
legitimate and shows that they bite: tests/test_gemm_parity_cpu.py.

The launch is recorded: every call runs between sdumc_profile_enable(1) and sdumc_profile_report, and the variant the test names must
have been launched, the expected number of times, and no other.  (frame_dx's split route has no profile hook: its runs assert that
NOTHING was recorded -- the fp32-MFMA route it would otherwise have taken records a generic launch -- and the launcher's dispatch on
split bit 1 names the kernel.)

Operands are views into larger allocations with the row stride above the extent wherever the header allows it; everything outside the
logical extent is NaN: the padding columns, the rows behind the last one (behind a_row_mod), the rows of a packed store that no map
entry names (its all-zero row stays zero), the rows of dz behind a sample's length.  The workspace is exactly as large as the query
says, NaN-filled, with a guard behind it.  Outputs are views with ldc above N: NaN inside (the known C0 with `accumulate`), a fixed int32
pattern in the padding columns and in a band of rows behind, which must be untouched afterwards.
Each run prints one `gemm route` line (worst slice beside its e_ref and bar): profiles/gemm_parity_by_route.txt."""
import ctypes as C
import os

import pytest
import torch

from tests import gemm_cases as GC

pytestmark = pytest.mark.gpu
PATTERN = 0x5A5AA5A5
NAN = float("nan")
SPLIT_BIT = {"group": 1, "f32": 2, "dx": 2, "rows": 8}


@pytest.fixture(scope="module")
def env():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from sdumc_amd import ops, _lib
    return ops, _lib


def up(n, q):
    return (n + q - 1) // q * q


def view2d(t, q, dtype=torch.float32, ld=None, fill=NAN):
    """t [rows, cols] -> a device view of a larger NaN-filled allocation: row stride up(cols, q) + q (or ld), three rows behind"""
    rows, cols = t.shape
    ld = ld or up(cols, q) + q
    big = torch.full((rows + 3, ld), fill, dtype=dtype, device="cuda")
    big[:rows, :cols] = t.to(dtype)
    return big[:rows, :cols]


def bytes2d(rows, cols, pad, fill=255):
    """uint8 [rows, cols] view with row stride cols + pad, three rows behind, filled with 0xff (NaN as fp32 / bf16, keep-everything as bits)"""
    big = torch.full((rows + 3, cols + pad), fill, dtype=torch.uint8, device="cuda")
    return big[:rows, :cols]


class Out:
    """an output [M, N] of `dtype` as a view into an int32-patterned allocation: ld = up(N, q) + q, four guard rows behind"""

    def __init__(self, M, N, q, dtype=torch.float32, C0=None):
        per = 4 // torch.empty(0, dtype=dtype).element_size()
        self.ld = up(up(N, q) + q, per)
        self.M, self.N, self.dtype = M, N, dtype
        self.raw = torch.full(((M + 4) * self.ld // per,), PATTERN, dtype=torch.int32, device="cuda")
        self.t = self.raw.view(dtype).view(M + 4, self.ld)[:M, :N]
        if C0 is None:
            self.t.fill_(255 if dtype == torch.uint8 else NAN)
        else:
            self.t.copy_(C0.to(dtype))

    def intact(self):
        chk, want = self.raw.clone(), torch.full_like(self.raw, PATTERN)
        for x in (chk, want):
            x.view(self.dtype).view(self.M + 4, self.ld)[:self.M, :self.N] = 0
        return torch.equal(chk, want)


class Workspace:
    """exactly `need` NaN bytes, a guard of 256 pattern bytes behind"""

    def __init__(self, need):
        self.need = int(need)
        self.raw = torch.full((up(self.need, 16) + 256,), 0xA5, dtype=torch.uint8, device="cuda")
        self.raw[:self.need] = 255
        self.t = self.raw[:self.need]

    def ptr(self):
        return self.raw.data_ptr()

    def intact(self):
        return bool((self.raw[self.need:] == 0xA5).all())


def vec_out(n, c0=None):
    return Out(1, n, 4, C0=None if c0 is None else c0.reshape(1, n))


def dev(t, dtype=None):
    return None if t is None else (t.to(dtype) if dtype else t).cuda().contiguous()


# ---- one driver per entry point: -> (call, outputs per problem as name -> device tensor, guards) -----------------------------------
def drive_f32(ops, _lib, r):
    o, probs = r["opts"], r["probs"]
    p = probs[0]
    lay, batch = p["layout"], o.get("batch", 0)
    q = 4 if ("wide" in r["variant"] or o.get("bf16")) else 1
    Is = [GC.operands(r, i) for i in range(len(probs))]
    g = _lib.Gemm()
    g.layout, g.M, g.N, g.K, g.groups = lay, p["M"], p["N"], p["K"], 1 if batch else len(probs)
    keep, outs, guards = [], [], []

    def place(ts):          # one allocation for the entries of a batch (-> views, stride in floats), else one each
        if not batch:
            return [view2d(t, q) for t in ts], 0
        rows, cols = ts[0].shape
        big = view2d(torch.cat([torch.cat([t, torch.full((2, cols), NAN)]) for t in ts]), q)
        return [big[z * (rows + 2):z * (rows + 2) + rows] for z in range(len(ts))], (rows + 2) * big.stride(0)
    As, g.stride_a = place([I["A"][0] for I in Is])
    Bs, g.stride_b = place([I["B"][0] for I in Is])
    g.lda, g.ldb = As[0].stride(0), Bs[0].stride(0)
    if batch:
        co = Out(batch * (p["M"] + 2) - 2, p["N"], q)
        Cs = [co.t[z * (p["M"] + 2):z * (p["M"] + 2) + p["M"]] for z in range(batch)]
        g.stride_c, g.batch = (p["M"] + 2) * co.ld, batch
        guards.append(co)
        g.A[0], g.B[0], g.C[0], g.ldc = As[0].data_ptr(), Bs[0].data_ptr(), Cs[0].data_ptr(), co.ld
        outs = [{"C": c} for c in Cs]
    for i, I in enumerate(Is if not batch else []):
        co = Out(p["M"], p["N"], q, C0=I.get("C0"))
        g.A[i], g.B[i], g.C[i], g.ldc = As[i].data_ptr(), Bs[i].data_ptr(), co.t.data_ptr(), co.ld
        guards.append(co)
        out = {"C": co.t}
        if p["bias"]:
            keep.append(dev(I["bias"]))
            g.bias[i] = keep[-1].data_ptr()
        if p["colsum"]:
            cs = vec_out(p["M"], I.get("cs0"))
            g.colsum_a[i], out["colsum"] = cs.t.data_ptr(), cs.t
            guards.append(cs)
        if p["keep"]:          # the descriptor only says "enabled, scale 2, this width": the mask is the attached keep-bits
            rows, width = I["keep"].shape
            bits = bytes2d(rows, width // 4, 0)
            bits.copy_(GC.pack_bits(I["keep"]))
            d = _lib.make_dropout(True, 0, 0.5, rows, width, 1)
            if p["keep"] == "A":
                g.a_drop = d
            else:
                g.b_drop = d
            g.ab_drop_bits[i] = bits.data_ptr()
            keep.append(bits)
        if p["masky"]:
            keep.append(view2d(I["Y"], q, ld=co.ld))
            g.c_mask_y[i], g.c_mask_scale = keep[-1].data_ptr(), I["mask_scale"]
        outs.append(out)
    g.a_row_mod, g.b_row_mod = p["amod"], p["bmod"]
    g.act, g.accumulate, g.splitk, g.tile, g.bf16 = p["act"], int(p["acc"]), o.get("splitk", 1), o.get("tile", 0), int(bool(o.get("bf16")))
    ws = Workspace(_lib.lib.sdumc_gemm_workspace_bytes(C.byref(g)))
    g.workspace, g.workspace_bytes = ws.ptr(), ws.need
    keep += [As, Bs, g]
    return (lambda: _lib.check(_lib.lib.sdumc_gemm_f32(C.byref(g), _lib.current_stream()), "sdumc_gemm_f32")), outs, guards + [ws], keep


def drive_bf16(ops, _lib, r):
    o, p, I = r["opts"], r["probs"][0], GC.operands(r, 0)
    bf = torch.bfloat16
    g = _lib.GemmBf16()
    g.layout, g.M, g.N, g.K, g.groups = p["layout"], p["M"], p["N"], p["K"], 1
    A, B = view2d(I["A"][0], 8, bf), view2d(I["B"][0], 8, bf)
    co = Out(p["M"], p["N"], 8, bf if p["bf16out"] else torch.float32, C0=I.get("C0"))
    g.A[0], g.B[0], g.C[0], g.lda, g.ldb, g.ldc = A.data_ptr(), B.data_ptr(), co.t.data_ptr(), A.stride(0), B.stride(0), co.ld
    keep, guards, out = [A, B, g], [co], {"C": co.t}
    if p["bias"]:
        keep.append(dev(I["bias"]))
        g.bias[0] = keep[-1].data_ptr()
    if p["colsum"]:
        cs = vec_out(p["M"], I.get("cs0"))
        g.colsum_a[0], out["colsum"] = cs.t.data_ptr(), cs.t
        guards.append(cs)
    g.a_row_mod, g.b_row_mod, g.act, g.accumulate, g.c_bf16, g.splitk = p["amod"], p["bmod"], p["act"], int(p["acc"]), int(p["bf16out"]), o.get("splitk", 0)
    ws = Workspace(_lib.lib.sdumc_gemm_bf16_workspace_bytes(C.byref(g)))
    g.workspace, g.workspace_bytes = ws.ptr(), ws.need
    return (lambda: _lib.check(_lib.lib.sdumc_gemm_bf16_run(C.byref(g), _lib.current_stream()), "sdumc_gemm_bf16_run")), [out], guards + [ws], keep


def store_of(rows_virtual, m, S, zero_row, dtype, q):
    """the packed store of a row map: S rows, NaN but the rows the map names and the all-zero row"""
    st = torch.full((S, rows_virtual.shape[1]), NAN)
    st[zero_row] = 0.0
    st[m.long()] = rows_virtual
    return view2d(st, q, dtype)


def drive_group(ops, _lib, r):
    probs = r["probs"]
    hf = probs[0]["bf16"]
    dt, q = (torch.bfloat16, 8) if hf else (torch.float32, 4)
    n = len(probs)
    arr = (_lib.GGProblem * n)()
    keep, outs, guards = [arr], [], []
    for i, p in enumerate(probs):
        I, g = GC.operands(r, i), arr[i]
        g.M, g.N = p["M"], p["N"]
        k0 = 0
        for s, k in enumerate(I["Ks"]):
            A = view2d(I["A"][s], q, dt)
            if p["bmap"]:
                m, S, z = I["maps"][s]
                B = store_of(I["B"][s], m, S, z, dt, q)
                keep.append(torch.cat([m, torch.zeros(4, dtype=torch.int32)]).cuda())      # (the bf16 form fetches entries four at a time)
                g.b_map[s] = keep[-1].data_ptr()
            else:
                B = view2d(I["B"][s], q, dt)
            g.A[s], g.B[s], g.K[s], g.lda, g.ldb = A.data_ptr(), B.data_ptr(), k, A.stride(0), B.stride(0)
            g.b_row_mod[s] = p["bmod1" if s else "bmod"]
            if p["keep"]:
                bits = bytes2d(k, p["N"] // 4, 4)
                bits.copy_(GC.pack_bits(I["keep"][k0:k0 + k]))
                g.b_bits[s], g.bits_qw, g.b_scale = bits.data_ptr(), bits.stride(0), I["scale"]
                keep.append(bits)
            keep += [A, B]
            k0 += k
        co = Out(p["M"], p["N"], 4, C0=I.get("C0"))
        g.C, g.ldc, g.accumulate = co.t.data_ptr(), co.ld, int(p["acc"])
        guards.append(co)
        out = {"C": co.t}
        if p["colsum"]:
            cs = vec_out(p["M"], I.get("cs0"))
            g.colsum_a, out["colsum"] = cs.t.data_ptr(), cs.t
            guards.append(cs)
        outs.append(out)
    lib = _lib.lib
    ws = Workspace((lib.sdumc_gemm_group_bf16_workspace_bytes if hf else lib.sdumc_gemm_group_workspace_bytes)(arr, n))
    fn = lib.sdumc_gemm_group_tn_bf16 if hf else lib.sdumc_gemm_group_tn
    return (lambda: _lib.check(fn(arr, n, ws.ptr(), ws.need, _lib.current_stream()), "sdumc_gemm_group_tn")), outs, guards + [ws], keep


def nt_operand(ops, p, I, to_store, pad):
    """A (and A2, and the maps) of the p3 / b1 NT product: to_store(fp32 rows [n, K]) -> a device view in the entry point's storage.
    -> (A, A2 or None, a_map, a2_map, rows of the larger store)"""
    A = I["A"][0]
    if not p["amap"]:
        return to_store(A[:p["a2"]] if p["a2"] else A), (to_store(A[p["a2"]:]) if p["a2"] else None), None, None, 0
    parts = [A[:p["a2"]], A[p["a2"]:]] if p["a2"] else [A]
    st, maps = [], []
    for rows, (m, S, z) in zip(parts, I["maps"]):
        full = torch.full((S, A.shape[1]), NAN)
        full[z] = 0.0
        full[m.long()] = rows
        st.append(to_store(full))
        maps.append(m.cuda())
    return st[0], (st[1] if p["a2"] else None), maps[0], (maps[1] if p["a2"] else None), max(S for _, S, _ in I["maps"])


def drive_p3(ops, _lib, r):
    o, p, I = r["opts"], r["probs"][0], GC.operands(r, 0)
    M, N, K = p["M"], p["N"], p["K"]

    def to_store(x):          # fp32 [n, K] -> P3 rows of 6 K bytes at a stride of 6 K + 32, NaN planes around
        out = bytes2d(x.shape[0], 6 * K, 32)
        return ops.p3_split(x.cuda().contiguous(), out=out)
    A, A2, amap, a2map, S = nt_operand(ops, p, I, to_store, 32)
    B3 = ops.p3_split_frag(dev(I["B"][0]))
    g = _lib.GemmP3()
    g.M, g.N, g.K, g.A, g.B, g.lda, g.ldb = M, N, K, A.data_ptr(), B3.data_ptr(), A.stride(0), B3.stride(0)
    g.a_row_mod = p["amod"]
    keep, guards = [A, A2, B3, amap, a2map, g], []
    if A2 is not None:
        g.A2, g.a2_row0 = A2.data_ptr(), p["a2"]
    if amap is not None:
        g.a_map, g.a_map_rows = amap.data_ptr(), S if o.get("map_rows") else 0
        if a2map is not None:
            g.a2_map = a2map.data_ptr()
    if p["keep"]:
        bits = bytes2d(M, K // 4, 4)
        bits.copy_(GC.pack_bits(I["keep"]))
        g.a_bits, g.bits_qw, g.a_scale = bits.data_ptr(), bits.stride(0), I["scale"]
        keep.append(bits)
    if p["bias"]:
        keep.append(dev(I["bias"]))
        g.bias = keep[-1].data_ptr()
    co = Out(M, N, 4)
    g.act, g.C, g.ldc, g.splitk, g.tile_m = p["act"], co.t.data_ptr(), co.ld, o.get("splitk", 0), o.get("tile_m", 0)
    guards.append(co)
    cp = None
    if o.get("want_p3"):
        cp = Out(M, 6 * N, 16, torch.uint8)
        g.C_p3, g.ldc_p3 = cp.t.data_ptr(), cp.ld
        guards.append(cp)
    ws = Workspace(_lib.lib.sdumc_gemm_p3_workspace_bytes(C.byref(g)))
    g.workspace, g.workspace_bytes = ws.ptr(), ws.need
    out = {"C": co.t}
    if cp is not None:
        out["C_p3"] = cp.t
    return (lambda: _lib.check(_lib.lib.sdumc_gemm_p3_nt(C.byref(g), _lib.current_stream()), "sdumc_gemm_p3_nt")), [out], guards + [ws], keep


def drive_b1(ops, _lib, r):
    o, p, I = r["opts"], r["probs"][0], GC.operands(r, 0)
    M, N, K = p["M"], p["N"], p["K"]
    bf = torch.bfloat16
    A, A2, amap, a2map, S = nt_operand(ops, p, I, lambda x: view2d(x, 8, bf), 8)
    Bf = ops.b1_frag(dev(I["B"][0]))
    g = _lib.GemmB1()
    g.M, g.N, g.K, g.A, g.B, g.lda, g.ldb = M, N, K, A.data_ptr(), Bf.data_ptr(), A.stride(0), Bf.stride(0)
    g.a_row_mod = p["amod"]
    keep = [A, A2, Bf, amap, a2map, g]
    if A2 is not None:
        g.A2, g.a2_row0 = A2.data_ptr(), p["a2"]
    if amap is not None:
        g.a_map, g.a_map_rows = amap.data_ptr(), S if o.get("map_rows") else 0
        if a2map is not None:
            g.a2_map = a2map.data_ptr()
    if p["bias"]:
        keep.append(dev(I["bias"]))
        g.bias = keep[-1].data_ptr()
    co = Out(M, N, 8, bf if p["bf16out"] else torch.float32)
    g.act, g.C, g.ldc, g.c_bf16, g.splitk = p["act"], co.t.data_ptr(), co.ld, int(p["bf16out"]), o.get("splitk", 0)
    ws = Workspace(_lib.lib.sdumc_gemm_b1_workspace_bytes(C.byref(g)))
    g.workspace, g.workspace_bytes = ws.ptr(), ws.need
    return (lambda: _lib.check(_lib.lib.sdumc_gemm_b1_nt(C.byref(g), _lib.current_stream()), "sdumc_gemm_b1_nt")), [{"C": co.t}], [co, ws], keep


def drive_rows(ops, _lib, r):
    probs = r["probs"]
    hf = probs[0]["bf16"]
    dt, q = (torch.bfloat16, 8) if hf else (torch.float32, 4)
    qs, outs, guards = [], [], []
    for i, p in enumerate(probs):
        I = GC.operands(r, i)
        co = Out(GC.out_rows(p), 256, q, dt, C0=I.get("C0"))
        d = {"A": view2d(I["A"][0], q, dt), "B": view2d(I["B"][0], q, dt), "M": p["M"], "a_row_mod": p["amod"], "C": co.t,
             "accumulate": p["acc"], "act": p["act"], "bias": dev(I.get("bias"))}
        if p["keep"]:
            d["bits"], d["scale"] = dev(GC.pack_bits(I["keep"])), I["scale"]
        if p["pool"]:
            d["pool_w"], d["pool_g"], d["pool_T"], d["fold"] = dev(I["pool_w"]), dev(I["pool_g"]), p["pool"][0], p["fold"]
            if p["cbits"]:
                d["c_bits"], d["c_scale"] = dev(GC.pack_bits(I["ckeep"])), I["c_scale"]
        qs.append(d)
        outs.append({"C": co.t})
        guards.append(co)
    return (lambda: ops.gemm_rows256(qs)), outs, guards, qs


def drive_dx(ops, _lib, r):
    o, p, I = r["opts"], r["probs"][0], GC.operands(r, 0)
    M, N = p["M"], p["N"]
    dz = I["A"][0].clone()
    dz[GC.zero_rows(p)] = NAN                        # rows behind a sample's length are not multiplied, whatever they hold
    big = torch.full((M + 3, 256), NAN, device="cuda")
    big[:M] = dz.cuda()
    W = view2d(I["B"][0], 4)
    co = Out(M, N, 4)
    lengths = dev(torch.tensor(p["lens"][1], dtype=torch.int32)) if p["lens"] else None
    ws = Workspace(_lib.lib.sdumc_frame_dx_scratch_bytes(N))
    W_frag = ops.p3_split_frag_t(W) if o.get("packed") else None
    call = lambda: ops.frame_dx(big[:M], W, C_out=co.t, W_frag=W_frag, lengths=lengths, T=p["lens"][0] if p["lens"] else 0, scratch=ws.t)
    return call, [{"C": co.t}], [co, ws], [big, W, W_frag, lengths]


DRIVE = dict(f32=drive_f32, bf16=drive_bf16, group=drive_group, p3=drive_p3, b1=drive_b1, rows=drive_rows, dx=drive_dx)


def recorded(_lib, call):
    """variant name -> launches of everything `call` launched through the GEMM entry points"""
    lib = _lib.lib
    torch.cuda.synchronize()
    lib.sdumc_profile_enable(1)
    try:
        call()
        torch.cuda.synchronize()
        arr = (_lib.ProfEntry * 32)()
        n = lib.sdumc_profile_report(arr, 32)
    finally:
        lib.sdumc_profile_enable(0)
    assert n > 0, "sdumc_profile_report failed"
    return {arr[i].name.decode(): int(arr[i].launches) for i in range(n) if arr[i].launches}


def check_run(env, rid):
    try:
        return _check_run(env, rid)
    except RuntimeError as e:          # a HIP error leaves the device in an unknown state: the session starts nothing more on it
        if any(w in str(e) for w in ("ELAUNCH", "HIP error", "illegal memory", "hipError")):
            pytest.exit("%s: %s" % (rid, e), returncode=3)
        raise


def _check_run(env, rid):
    ops, _lib = env
    r = GC.by_id(rid)
    default = int(os.environ.get("SDUMC_SPLIT", "15"))
    try:
        if "split" in r["opts"]:
            bit = SPLIT_BIT[r["entry"]]
            _lib.lib.sdumc_set_split_((default | bit) if r["opts"]["split"] else (default & ~bit))
        call, outs, guards, keep = DRIVE[r["entry"]](ops, _lib, r)
        seen = recorded(_lib, call)
    finally:
        _lib.lib.sdumc_set_split_(default)
    if "cut" in r["opts"]:          # the plan really cut K over workgroups (slabs in the workspace), or really did not
        need = [x.need for x in guards if isinstance(x, Workspace)][0]
        assert (need > 0) == r["opts"]["cut"], "%s: workspace query %d bytes" % (rid, need)
    want = {r["variant"]: r["launches"]} if r["launches"] else {}
    assert seen == want, "%s: launched %s, the route is %s" % (rid, seen, want)
    got = []
    for i, out in enumerate(outs):
        p = r["probs"][i]
        g = {k: v.float().cpu() for k, v in out.items() if k != "C_p3"}
        if "C_p3" in out:         # the P3 copy of the output, joined: the same values, the same bar
            joined = ops.p3_join(out["C_p3"], p["N"])
            assert torch.equal(joined, out["C"]), "%s: C_p3 is not the split of C" % rid
        if p["lens"]:
            z = GC.zero_rows(p)
            assert int(torch.count_nonzero(g["C"][z].view(torch.int32))) == 0, "%s: rows behind a sample's length are not +0.0" % rid
        got.append(g)
    res, line = GC.judge(r, got)
    for x in guards:
        assert x.intact(), "%s: a guard of %s was written" % (rid, type(x).__name__)
    del keep
    return res


def _route_test(variant):
    ids = [r["id"] for r in GC.RUNS if r["variant"] == variant]

    @pytest.mark.parametrize("rid", ids, ids=[GC.by_id(i)["name"] for i in ids])
    def test(env, rid):
        check_run(env, rid)
    test.__name__ = test.__qualname__ = "test_" + variant
    test.__doc__ = "the runs of tests/gemm_cases.py whose launch the profile reports as %s" % variant
    return test


for _v in dict.fromkeys(r["variant"] for r in GC.RUNS):
    globals()["test_" + _v] = _route_test(_v)
