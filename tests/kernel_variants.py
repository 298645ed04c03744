"""The kernel variants of the dense layers (csrc/linear.hip, mlp.hip, attention.hip) and of the fused point layers (fusion.hip,
cross.hip, pointconv.hip, ptblock.hip), the backward units of the fused point layers (fusion_grad.hip, cross_grad.hip,
cross256_grad.hip, pointconv_grad.hip, ptblock_grad.hip), and the parity cases that reach them.

expected_kernel() mirrors the C dispatch: given an entry point and a shape it names the template instantiation that runs, in
the form c++filt prints it without namespace and arguments ("linear_kernel<3, 2, 8>").  CASES parametrises
test_kernel_variants_gpu.py (dense layers) and test_fused_variants_gpu.py (point layers); test_kernel_variants_cpu.py checks that every instantiation in the device assembly is named by at
least one case, so a variant added later without a parity case fails the CPU suite.

expected_grad_kernels() names the set of kernels one backward call launches and grad_launch_grid() mirrors how each of them deals
its points (or point pairs) to workgroups; GRAD_CASES parametrises test_fused_grad_variants_gpu.py, and test_kernel_variants_cpu.py
checks that they reach every kernel the backward units emit and every edge of their persistent loops.  BN_CASES,
expected_bn_kernels() and bn_launch_grid() do the same for the train-mode fusion layer (fusion_bn.hip, forward and backward in one
unit, two grid caps in one call) and parametrise test_fusion_bn_variants_gpu.py.

wgrad_launch() restates the host dispatch of the weight-gradient kernel (linear_grad.hip: tiles-per-wave variant, stages per
workgroup, idle workgroups, how each operand is staged); WGRAD_CASES parametrises test_linear_grad_edges_gpu.py.
attention_small_grad_launch() does the same for the three narrow-head attention backward kernels (attention_grad.hip) and
ATTN_GRAD_COUNTS is the grid of query / key counts test_attention_grad_edges_gpu.py crosses.

attention_wide_train_kernels() names the kernels one training forward + backward of the wide-head attention launches
(attention_wide_grad.hip, 43 instantiations) and attention_wide_grad_launch() mirrors their tiles and stages; WIDE_GRAD_COUNTS,
WIDE_GUARD_CASES and WIDE_TRAIN_CASES parametrise test_attention_wide_grad_edges_gpu.py.  EMD_GRAD_CASES and INTERP3_GRAD_CASES are
the shapes of test_emd_interp3_grad_edges_gpu.py, each with the kernels it launches.

primitive_launch() restates the host side of every C entry of the oldest units (pointnet2_ops.hip, interp3.hip, norm.hip: gathers,
scatters, the 3-NN blend, the row normalisation) -- instantiation, grid, grid-stride rounds, the live items of the last round and of
the last workgroup, with the alignment of the operands as an input; PRIMITIVE_CASES parametrises test_primitive_edges_gpu.py and
test_primitive_variants_cpu.py holds it to the units' device assembly.  A plain module, imported by the tests."""

def _cdiv(a, b):
    return (a + b - 1) // b


LINEAR_SPLITK_ROWS = 16384  # MCP_LINEAR_SPLITK_ROWS, csrc/linear.hip:24


def _linear(rows, ks, n, policy_rows=None):
    nt, total = _cdiv(n, 32), sum(_cdiv(k, 32) for k in ks)          # mcp_linear_as, linear.hip:551 (count_chunks :493-497)
    if nt in (5, 7) or (nt > 8 and nt % 4):                          # mcp_linear_packed_floats, linear.hip:522-523
        raise ValueError(f"linear: n={n} is not built")
    prows = rows if policy_rows is None else policy_rows
    if prows < LINEAR_SPLITK_ROWS and total >= 4:                    # linear.hip:554-556
        return f"linear_splitk_kernel<{1 if nt & 1 else 2}>"
    if nt > 8:                                                       # linear.hip:567 -> launch_linear_blocked :421-426
        nt_k, nw = 4, 8 if rows >= 131072 else 4
    elif nt > 4:                                                     # launch_linear, linear.hip:432
        nt_k, nw = nt, 4
    else:                                                            # linear.hip:434-435 (the row count, not policy_rows)
        nt_k, nw = nt, 8 if rows >= 131072 else 4
    kc = 4 if nt_k <= 2 else 2 if nt_k <= 4 else 1                   # launch_linear_nw, linear.hip:415
    if not (kc > 1 and total >= 2 * kc):                             # linear.hip:416-418
        kc = 1
    return f"linear_kernel<{nt_k}, {kc}, {nw}>"


def _linear_narrow(k, n, rows=None):
    if n < 1 or n > 4 or k not in (256, 512, 1024):                  # mcp_linear_narrow, linear.hip:504
        raise ValueError(f"linear_narrow: k={k}, n={n} is not built")
    return f"linear_narrow_kernel<{k // 256}>"                        # linear.hip:510-512


def _mlp2(rows, cin, hidden, cout):
    cot = _cdiv(cout, 32)
    if not (hidden > 0 and hidden % 32 == 0 and ((cin == 64 and cot in (1, 2)) or (cin == 128 and cot in (1, 4)))):
        raise ValueError(f"mlp2: {cin}-{hidden}-{cout} is not built")  # supported(), mlp.hip:176-183
    cot_k = cot                                                      # mlp.hip:217-220
    nw = 4 if rows < 32768 else 8                                    # MLP2_GO, mlp.hip:214-216
    return f"mlp2_kernel<{cin}, {cot_k}, {nw}>"


def _attention(bf, nq, nk, heads, hd):
    if hd in (8, 16):                                                # attention_forward_run, csrc/attention_forward.h
        return f"attention_small_kernel<{hd}>"
    if hd in (32, 64):                                               # attention_forward_run: widths 32 / 64 never split the keys
        return f"attention_wide_kernel<{hd}>"
    if hd == 256:                                                    # attention_forward_run: wide_keys_split
        if _cdiv(nq, 128) * heads * bf * 4 < 1024 and nk >= 128:
            return "attention_wide_ksplit_kernel<256>"
        return "attention_wide_kernel<256>"
    raise ValueError(f"attention: head width {hd} is not built")      # mcp_attention, attention.hip


# ---- the fused point layers.  launch_grid() mirrors the grid arithmetic beside each dispatch, so that test_kernel_variants_cpu.py can
# check that the cases reach the loop edges their comments name ----
POINTCONV_LOWLEVEL_MAX = 16384   # pc_agg_run, csrc/pointconv_tile.h
FUSION_WAVES, FUSION_GRID_CAP = 4, 4096                      # fusion.hip:34, :298
CROSS_WAVES = {64: 4, 128: 8, 256: 4}                        # CrossShape<D>::NW, cross.hip; X256_WAVES, cross_tile.h
CROSS_GRID_CAP = {64: 768, 128: 256, 256: 256}               # CrossShape<D>::GRID and launch_cross256, cross.hip
PTBLOCK_WAVES, PTBLOCK_GRID_CAP = 4, 768                     # ptblock.hip:19, :194


def _fusion(b, n, nb=64):
    if nb != 64:                                                     # mcp_fusion, fusion.hip:291
        raise ValueError(f"fusion: {nb} neighbours are not built")
    return "fusion_split_kernel"                                     # fusion.hip:318 (fusion_kernel only under -DMCP_AB, :306-312)


def _cross(d, k=32):
    if k != 32 or d not in (64, 128, 256):                           # mcp_cross_volume, cross.hip
        raise ValueError(f"cross: d={d}, k={k} is not built")
    if d == 256:                                                     # mcp_cross_volume -> launch_cross256
        return "cross256_stream_kernel"
    return f"cross_kernel<{d}, 1>"                                   # launch_cross<D, 1>, cross.hip


def _pointconv_agg(b, s, d, aligned=True, k=32):
    if k != 32:                                                      # pc_agg_run, csrc/pointconv_tile.h
        raise ValueError(f"pointconv_agg: {k} neighbours are not built")
    total = b * s
    vec4 = d % 4 == 0 and aligned                                    # pc_agg_run: vec4 (aligned: s_points on a 16-byte boundary)
    if total <= POINTCONV_LOWLEVEL_MAX or not vec4:                  # pc_agg_run: the low-level forms
        if d >= 256 and total <= 8192:                               # pc_agg_run
            return "pointconv_agg_lowlevel_kernel<1024>"
        return "pointconv_agg_lowlevel_kernel<256>"                  # pc_agg_run
    if d <= 32:                                                      # pc_agg_run: points per workgroup by d
        return "pointconv_agg_kernel<256, 32>"
    if d <= 64:                                                      # pc_agg_run
        return "pointconv_agg_kernel<256, 16>"
    return "pointconv_agg_kernel<256, 8>"                            # pc_agg_run


def _pointconv_linear(d, c_out, k=32):
    if k != 32 or (d, c_out) not in ((32, 32), (64, 64)):            # pc_linear_run, csrc/pointconv_tile.h
        raise ValueError(f"pointconv_linear: d={d}, c_out={c_out}, k={k} is not built")
    return "pointconv_linear_kernel<32, 1>" if d == 32 else "pointconv_linear_kernel<64, 2>"   # pc_linear_run


def _ptblock(c=64, k=16):
    if c != 64 or k != 16:                                           # mcp_ptblock_attention, ptblock.hip:188
        raise ValueError(f"ptblock: c={c}, k={k} is not built")
    return "ptblock_kernel"                                          # ptblock.hip:197


def launch_grid(op, **shape):
    """(workgroups, units, units per workgroup step) of the launch: `units` are what the kernel's persistent loop deals out (points,
    or point pairs in ptblock_kernel).  mcp_units_by_xcd (common.h) and cross_kernel (its own deal, cross.hip) deal units by XCD
    when the grid is a multiple of 8; cross256_stream_kernel always deals round-robin (its `rounds`, cross.hip)."""
    if op == "fusion":                                               # fusion.hip:304
        total = shape["b"] * shape["n"]
        return min(_cdiv(total, FUSION_WAVES), FUSION_GRID_CAP), total, FUSION_WAVES
    if op == "cross":
        d, total = shape["d"], shape["b"] * shape["n1"]
        nw = CROSS_WAVES[d]
        want = _cdiv(total, nw) if d == 256 else _cdiv(total, nw * 8)   # launch_cross256, launch_cross
        return max(1, min(want, CROSS_GRID_CAP[d])), total, nw          # launch_cross256, launch_cross
    if op == "pointconv_agg":
        total = shape["b"] * shape["s"]
        name = expected_kernel(op, **shape)
        ppb = 8 if "lowlevel" in name else int(name[:-1].split(",")[1])  # LPPB, pointconv_tile.h; PPB: pc_agg_run
        return min(_cdiv(total, ppb), 1 << 20), total, ppb              # pc_agg_run: the launch lambda's grid
    if op == "pointconv_linear":                                     # FPPB, pointconv_tile.h; pc_linear_run's grid
        total = shape["b"] * shape["s"]
        return min(_cdiv(total, 32), 1 << 20), total, 32
    if op == "ptblock":                                              # ptblock.hip:103, :193-194
        pairs = (shape["b"] * shape["n"] + 1) // 2
        return max(1, min(_cdiv(pairs, PTBLOCK_WAVES * 4), PTBLOCK_GRID_CAP)), pairs, PTBLOCK_WAVES
    raise ValueError(f"unknown op {op}")


def expected_kernel(op, **shape):
    """Demangled name of the kernel the entry point `op` launches for `shape` (extra keys of a case are ignored):
    linear (rows, ks, n[, policy_rows]), linear_narrow (k, n), mlp2 (rows, cin, hidden, cout), attention (bf, nq, nk, heads, hd),
    fusion (b, n), cross (d), pointconv_agg (b, s, d[, aligned]), pointconv_linear (d, c_out), ptblock ()."""
    if op == "fusion":
        return _fusion(shape["b"], shape["n"], shape.get("nb", 64))
    if op == "cross":
        return _cross(shape["d"], shape.get("k", 32))
    if op == "pointconv_agg":
        return _pointconv_agg(shape["b"], shape["s"], shape["d"], shape.get("aligned", True), shape.get("k", 32))
    if op == "pointconv_linear":
        return _pointconv_linear(shape["d"], shape["c_out"], shape.get("k", 32))
    if op == "ptblock":
        return _ptblock(shape.get("c", 64), shape.get("k", 16))
    if op == "linear":
        return _linear(shape["rows"], shape["ks"], shape["n"], shape.get("policy_rows"))
    if op == "linear_narrow":
        return _linear_narrow(shape["k"], shape["n"])
    if op == "mlp2":
        return _mlp2(shape["rows"], shape["cin"], shape["hidden"], shape["cout"])
    if op == "attention":
        return _attention(shape["bf"], shape["nq"], shape["nk"], shape["heads"], shape["hd"])
    raise ValueError(f"unknown op {op}")


def _lin(rows, ks, n, slope=1.0, res=False, strided=False, policy_rows=None):
    return dict(op="linear", rows=rows, ks=tuple(ks), n=n, slope=slope, res=res, strided=strided, policy_rows=policy_rows)


def _mlp(rows, cin, hidden, cout, res=False, strided=False):
    return dict(op="mlp2", rows=rows, cin=cin, hidden=hidden, cout=cout, res=res, strided=strided)


def _att(bf, nq, nk, heads, hd, shift=None, logits=None, same_keys=False):
    """shift None: be.attention (kv packed as [k | v]); an int: be.attention_rot with that kv_shift.  logits: scale q so that
    max |q.k| * scale is about this.  same_keys: every key of head 0 identical."""
    return dict(op="attention", bf=bf, nq=nq, nk=nk, heads=heads, hd=hd, shift=shift, logits=logits, same_keys=same_keys)


def _fus(tag, b, n, **kw):
    """same: p2 is p1 (every list holds a zero-length vector); dup: the second list repeats the first; extent: coordinates of
    test_ops_gpu.cloud's extent; mutant=False: the output does not depend on the products (no two-term check)."""
    return dict(op="fusion", tag=tag, b=b, n=n, **kw)


def _crs(tag, d, b, n1, n2, **kw):
    return dict(op="cross", tag=tag, d=d, b=b, n1=n1, n2=n2, **kw)


def _agg(tag, b, n, s, d, **kw):
    """aligned=False: s_points is a view 4 bytes into its storage."""
    return dict(op="pointconv_agg", tag=tag, b=b, n=n, s=s, d=d, **kw)


def _pcl(tag, b, n, s, d, **kw):
    return dict(op="pointconv_linear", tag=tag, b=b, n=n, s=s, d=d, c_out=d, **kw)


def _ptb(tag, b, n, **kw):
    """packed: q, k, v are slices of one (B, N, 192) tensor in the checked run; logits: largest |attn| / 8; same: the 16 neighbours of a
    point are one point."""
    return dict(op="ptblock", tag=tag, b=b, n=n, **kw)


T8 = 131072 + 37    # 8-wave row count with a ragged last workgroup
T4 = 16384 + 5      # 4-wave row count with a ragged last tile

CASES = [
    # ---- linear_kernel<NT, KC, NW>: the tall path (rows >= 16384).  Comments: total K chunks against 2 * KC ----
    _lin(T8, (224,), 20, 0.1, strided=True),                 # <1,1,8>  7 chunks = 2*4 - 1
    _lin(T8, (256,), 1, 0.0, res=True),                      # <1,4,8>  8 chunks = 2*4, n = 1
    _lin(T8, (64, 36, 28), 33, 1.0),                         # <2,1,8>  three pieces, ragged middle piece
    _lin(196608, (536,), 64, 0.1),                           # <2,4,8>  the PointConv projection
    _lin(T8, (96,), 70, 0.0, res=True),                      # <3,1,8>  3 chunks = 2*2 - 1
    _lin(T8, (128,), 90, 0.1, strided=True),                 # <3,2,8>  4 chunks = 2*2
    _lin(T8, (64, 32), 97, 1.0, res=True),                   # <4,1,8>  two pieces
    _lin(T8, (132,), 128, 0.1),                              # <4,2,8>
    _lin(T8, (64,), 384, 0.0, res=True),                     # blocked <4,1,8>: 3 column blocks
    _lin(T8, (160,), 512, 0.1),                              # blocked <4,2,8>: 4 column blocks
    _lin(T4, (64,), 32, 1.0),                                # <1,1,4>
    _lin(T4, (100, 36, 128), 20, 0.1, res=True, strided=True),  # <1,4,4>  three pieces
    _lin(T4, (128,), 50, 0.0),                               # <2,1,4>  4 chunks < 2*4
    _lin(T4, (280,), 64, 0.1, res=True),                     # <2,4,4>
    _lin(T4, (32,), 65, 1.0),                                # <3,1,4>  one chunk
    _lin(T4, (200,), 96, 0.1, strided=True),                 # <3,2,4>
    _lin(T4, (64,), 100, 0.0),                               # <4,1,4>
    _lin(T4, (64, 64, 64), 128, 1.0, res=True),              # <4,2,4>
    _lin(T4, (96,), 170, 0.1, res=True),                     # <6,1,4>
    _lin(T4, (64, 36), 192, 0.0, strided=True),              # <6,1,4>  n = 192
    _lin(T8, (128,), 250, 0.1),                              # <8,1,4>  tall: NT > 4 stays on 4 waves
    _lin(T4, (96,), 384, 1.0),                               # blocked <4,1,4>
    _lin(T4, (256,), 512, 0.1, res=True),                    # blocked <4,2,4>
    # ---- linear_splitk_kernel<NT & 1 ? 1 : 2>: policy rows < 16384, >= 4 chunks ----
    _lin(20, (128,), 33, 0.1, res=True),                     # <2>  one ragged 32-row tile, exactly 4 chunks
    _lin(5000, (36, 64, 28), 20, 0.0, strided=True),         # <1>  three pieces
    _lin(3001, (256,), 96, 1.0),                             # <1>  NT = 3
    _lin(8191, (520,), 256, 0.1, res=True),                  # <2>  NT = 8
    # ---- linear_narrow_kernel<K / 256> ----
    dict(op="linear_narrow", rows=1024 + 3, k=256, n=1),
    dict(op="linear_narrow", rows=1024 + 3, k=512, n=2),
    dict(op="linear_narrow", rows=4099, k=1024, n=4),
    dict(op="linear_narrow", rows=2000, k=256, n=3),
    # ---- mlp2_kernel<CIN, COT, NW> around the 32768-row switch ----
    _mlp(32767, 64, 32, 1),                                  # <64,1,4>   one hidden chunk
    _mlp(32768, 64, 96, 3, res=True),                        # <64,1,8>   odd chunk count
    _mlp(32767, 64, 256, 64, res=True, strided=True),        # <64,2,4>
    _mlp(49152 + 3, 64, 512, 33, strided=True),              # <64,2,8>   the headline step's variant
    _mlp(1000, 128, 512, 32, res=True),                      # <128,1,4>
    _mlp(49152 + 3, 128, 96, 3),                             # <128,1,8>
    _mlp(20000, 128, 512, 128, res=True, strided=True),      # <128,4,4>
    _mlp(32768, 128, 32, 97),                                # <128,4,8>
    # ---- attention_wide_ksplit_kernel<256> (Cross_Frame_Att) ----
    _att(2, 37, 130, 1, 256),                                # partial last tile, dead query lanes
    _att(1, 100, 333, 3, 256),                               # 11 stages: 3/3/3/2 per wave
    _att(2, 256, 160, 3, 256),                               # 5 stages: 2/1/1/1
    _att(1, 64, 128, 2, 256),                                # one full stage per wave
    _att(2, 40, 129, 1, 256),                                # one live key in the last tile
    _att(2, 37, 130, 1, 256, shift=1),
    _att(3, 50, 200, 2, 256, shift=1),
    _att(3, 50, 200, 2, 256, shift=2),
    _att(2, 37, 130, 1, 256, logits=80.0),
    _att(2, 37, 160, 2, 256, same_keys=True),
    # ---- attention_wide_kernel<32 | 64 | 256> ----
    _att(2, 130, 20, 4, 32),                                 # nk < 32
    _att(1, 257, 200, 2, 32, shift=0),                       # nk % 64 != 0
    _att(3, 129, 31, 2, 64, shift=2),
    _att(1, 300, 100, 1, 64),
    _att(2, 130, 100, 2, 256),                               # nk < 128: no key split
    _att(3, 60, 90, 1, 256, shift=1),
    _att(2, 130, 100, 2, 32, logits=80.0),
    _att(2, 130, 100, 2, 64, logits=80.0),
    _att(2, 130, 100, 2, 256, logits=80.0),
    _att(2, 130, 70, 2, 32, same_keys=True),
    _att(2, 130, 70, 2, 64, same_keys=True),
    _att(2, 130, 70, 2, 256, same_keys=True),
    # ---- attention_small_kernel<8 | 16> ----
    _att(2, 1, 1, 8, 8),
    _att(1, 1, 31, 4, 8),
    _att(3, 200, 33, 8, 8, shift=1),
    _att(2, 1, 33, 8, 16),
    _att(1, 1, 1, 2, 16),
    _att(3, 130, 31, 8, 16, shift=2),
    _att(2, 130, 100, 8, 8, logits=80.0),
    _att(2, 130, 100, 8, 16, logits=80.0),
    _att(2, 130, 70, 8, 8, same_keys=True),
    _att(2, 130, 70, 8, 16, same_keys=True),
    # ---- fusion_split_kernel: one point per wave, 4 waves, grid = min(ceil(total / 4), 4096); by XCD when grid % 8 == 0 ----
    _fus("one-point", 1, 1, mutant=False),                   # 3 dead waves; the 64 neighbours are the one point: the blend is that point
    _fus("3-points", 1, 3),                                  # one workgroup, one dead wave
    _fus("5-points", 1, 5, same=True),                       # grid 2: the second workgroup has one live wave; zero-length vectors
    _fus("xcd-ragged", 1, 61),                               # grid 16: eighths of 8 points, the last one has 5
    _fus("grid-750", 2, 1499, same=True, dup=True),          # grid % 8 = 6: round-robin deal; p2 = p1 and every neighbour twice
    _fus("grid-cap-2-rounds", 3, 5483, extent=True),         # 16449 points on 4096 workgroups by XCD: 2060-point eighths, steps of 2048
    # ---- cross_kernel<64, 1>: 4 waves, grid = min(ceil(total / 32), 768) ----
    _crs("xcd-ragged", 64, 3, 83, 70, extent=True),          # (a, e) 249 points, grid 8: eighths of 32 cut inside batch elements, the last has 25
    _crs("grid-cap-stride>=n1", 64, 665, 37, 41),            # (b) 24605 points, grid 768 by XCD: steps of 384 points cross 10 batch elements
    _crs("grid-10", 64, 2, 150, 150),                        # (c) round-robin deal, steps of 40 < n1
    _crs("3-points", 64, 1, 3, 50),                          # (d) one workgroup, one wave without a point
    # ---- cross_kernel<128, 1>: 8 waves, grid = min(ceil(total / 64), 256) ----
    _crs("xcd-ragged", 128, 3, 167, 150, extent=True),       # (a, e) 501 points, grid 8: eighths of 63, the last has 60
    _crs("grid-cap-stride>=n1", 128, 443, 37, 41),           # (b) 16391 points, grid 256 by XCD: steps of 256 points cross 6 batch elements
    _crs("grid-10", 128, 2, 300, 300),                       # (c)
    _crs("5-points", 128, 1, 5, 50),                         # (d) three waves without a point
    # ---- cross256_stream_kernel: 4 waves in lockstep, grid = min(ceil(total / 4), 256), round-robin rounds ----
    _crs("ragged-workgroup", 256, 3, 83, 70, extent=True),   # (c, e) 249 points, grid 63: the last workgroup has one live wave
    _crs("grid-cap-3-rounds", 256, 59, 37, 41),              # (b) 2183 points, grid 256: rounds of 1024 cross 27 batch elements; 3 points in the last step
    _crs("3-points", 256, 1, 3, 50),                         # (d) the dead wave recomputes the last point and does not store
    # ---- pointconv_agg_lowlevel_kernel<256 | 1024>: 8 points per workgroup, one channel per thread ----
    _agg("total-16384", 4, 4096, 4096, 32),                  # the last total of the low-level route; S = N; grid 2048 by XCD
    _agg("d%4", 5, 3300, 3277, 5),                           # 16385 centres, d = 5: no float4 gather
    _agg("unaligned", 5, 3300, 3277, 32, aligned=False),     # 16385 centres, s_points 4 bytes off a 16-byte boundary
    _agg("wide-few", 2, 100, 77, 256, extent=True),          # <1024>: 154 centres, grid 20, the last workgroup has 2
    # ---- pointconv_agg_kernel<256, PPB>: PPB points per workgroup, (point, 4 channels) items ----
    _agg("total-16385", 5, 3300, 3277, 32, extent=True),     # <256,32> the first streaming total: grid 513, the last workgroup has 1 point
    _agg("d4=1", 5, 3327, 3327, 4),                          # <256,32> one item per point; S = N; grid 520 by XCD, the last workgroup has 27
    _agg("d=36", 5, 3300, 3277, 36),                         # <256,16> 9 items per point (144 of 256 threads), grid 1025
    _agg("d=64", 3, 6000, 5500, 64, extent=True),            # <256,16> grid 1032 by XCD, the last workgroup has 4 points
    _agg("d=128", 2, 8200, 8193, 128),                       # <256,8> 256 items: one round; grid 2049, the last workgroup has 2
    _agg("d=256", 1, 16445, 16445, 256),                     # <256,8> 512 items: two rounds; S = N; grid 2056 by XCD, the last workgroup has 5
    # ---- pointconv_linear_kernel<32, 1> / <64, 2>: 32 centres per workgroup ----
    _pcl("few", 1, 700, 333, 32),                            # 333 centres: the last group has 13
    _pcl("above-16384", 3, 6000, 5463, 32, extent=True),     # 16389 centres, grid 513: the last group has 5
    _pcl("few", 2, 515, 77, 64, extent=True),                # 154 centres: the last group has 26
    _pcl("above-16384", 2, 8200, 8200, 64),                  # 16400 centres, grid 513: the last group has 16
    # ---- ptblock_kernel: two points per wave, 4 waves, grid = min(ceil(pairs / 16), 768) ----
    _ptb("one-point", 1, 1),                                 # the odd tail alone: the second half-wave recomputes point 0
    _ptb("odd-B1", 1, 333, extent=True),                     # 167 pairs, grid 11 (round-robin), odd tail
    _ptb("odd-B3", 3, 111, packed=True),                     # 333 points: pairs straddle batch elements; q/k/v with row stride 192
    _ptb("grid-cap-odd", 3, 8183),                           # 24549 points, 12275 pairs on 768 workgroups by XCD: 4 rounds, ragged eighth, odd tail
    _ptb("xcd-ragged", 2, 117, logits=80.0),                 # 117 pairs in 30 steps on 8 workgroups: eighths of 4 steps, the last has 5 pairs; large logits
    _ptb("same-neighbour", 2, 125, same=True),               # a uniform softmax in every channel
]


def cases(op):
    return [c for c in CASES if c["op"] == op]


# ---- the backward units of the fused point layers.  Every backward kernel is persistent: one workgroup per CU at the most, units
# (points, or point pairs) dealt statically, weight-gradient partial vectors added by a second kernel over ALL workgroups ----
GRAD_WAVES = 4                    # WAVES, fusion_grad.hip:30, GradShape<D>::WAVES in cross_grad.hip, X256_WAVES in cross_tile.h, pointconv_grad.hip:18, ptblock_grad.hip
X256_DX_GRID, X256_W_SLICES, X256_W_PTS = 512, 64, 4     # DX_GRID, W_SLICES, W_PTS, cross256_grad.hip
X256_Z_GRID_CAP = 256             # plan(), cross256_grad.hip (a constant there, not the CU count)


def _deal(units, per, g, base=0, xcd_map=True):
    """(dealt by XCD, [workgroup][round] -> list of units) for g workgroups of one role that starts at workgroup `base` of the launch.
    mcp_units_by_xcd (common.h; base = 0) and cross_grad_kernel's deal() (cross_grad.hip): by XCD when g >= 8, g % 8 == 0 and base % 8 == 0
    -- eighths of ceil(steps / 8) whole steps, workgroup k starts at step k >> 3 of eighth k & 7 and strides g >> 3 steps --, else
    workgroup k starts at step k and strides g steps.  Wave w of a workgroup takes unit first + w + round * stride while below the limit
    (fusion_grad.hip:113, cross_grad_body's point loop in cross_grad.hip, pointconv_grad.hip:54, ptblock_grad.hip:149)."""
    by_xcd = xcd_map and g >= 8 and g % 8 == 0 and base % 8 == 0
    dealt = []
    for k in range(g):
        if by_xcd:
            chunk = _cdiv(_cdiv(units, per), 8) * per
            x = k & 7
            first, stride, limit = x * chunk + (k >> 3) * per, (g >> 3) * per, min((x + 1) * chunk, units)
        else:
            first, stride, limit = k * per, g * per, units
        dealt.append([list(range(f, min(f + per, limit))) for f in range(first, limit, stride)])
    return by_xcd, dealt


def _role(units, per, g, base=0, xcd_map=True):
    by_xcd, dealt = _deal(units, per, g, base, xcd_map)
    return dict(workgroups=g, units=units, per=per, by_xcd=by_xcd, dealt=dealt)


def grad_launch_grid(op, cus=256, **shape):
    """{role: dict(workgroups, units, per, by_xcd, dealt)} of one backward call on a device with `cus` compute units.  `units` are what
    the role's loop deals out -- points, or pairs of points (2 u, 2 u + 1) in pointconv_agg_grad_kernel and ptblock_grad_kernel --,
    `per` the units one workgroup takes per step, dealt[k][r] the units workgroup k takes in its round r (an empty dealt[k]: the
    workgroup receives nothing and still writes its partial vector)."""
    if op == "fusion":                                               # grad_grid, fusion_grad.hip:440-445
        total = shape["b"] * shape["n"]
        return {"points": _role(total, GRAD_WAVES, min(_cdiv(total, GRAD_WAVES), cus))}
    if op == "cross":
        d, total = shape["d"], shape["b"] * shape["n1"]
        want = _cdiv(total, GRAD_WAVES)
        if d == 64:                                                  # grad_grid<64>, cross_grad.hip (one role), cross_grad_kernel's deal
            return {"all": _role(total, GRAD_WAVES, min(want, cus))}
        if d == 128:                                                 # grad_grid<128>, cross_grad.hip; the roles of cross_grad_kernel
            g0, g1 = min(want, max(cus // 2, 1)), min(want, max(cus // 4, 1))
            return {"data": _role(total, GRAD_WAVES, g0, 0), "own0": _role(total, GRAD_WAVES, g1, g0), "own2": _role(total, GRAD_WAVES, g1, g0 + g1)}
        if d == 256:                                                 # plan(), cross256_grad.hip
            slices = min(_cdiv(total, 2 * X256_W_PTS), X256_W_SLICES)
            per = _cdiv(total, slices)                               # cross256_grad_w_kernel: slice s takes points s per .. (s + 1) per
            w = [[list(range(p, min(p + X256_W_PTS, total, (s + 1) * per))) for p in range(s * per, min((s + 1) * per, total), X256_W_PTS)]
                 for s in range(slices)]                             # in stages of W_PTS points, :195
            return {"z": _role(total, GRAD_WAVES, min(want, X256_Z_GRID_CAP), xcd_map=False),     # round-robin rounds, cross256_grad_z_kernel
                    "w": dict(workgroups=slices, units=total, per=X256_W_PTS, by_xcd=False, dealt=w),   # times 4 column blocks, :188, :429
                    "dx": _role(total, 1, min(total, X256_DX_GRID), xcd_map=False)}                 # cross256_grad_dx_kernel's point loop; plan()
        raise ValueError(f"cross grad: d={d} is not built")          # mcp_cross_grad, cross_grad.hip
    if op == "pointconv_agg":                                        # grad_grid, pointconv_grad_tile.h; pairs: the kernel's loop there
        total = shape["b"] * shape["s"]
        return {"pairs": _role((total + 1) // 2, GRAD_WAVES, min(_cdiv(total, 2 * GRAD_WAVES), cus))}
    if op == "ptblock":                                              # grad_grid, ptblock_grad.hip:417-421; pairs :147
        pairs = (shape["b"] * shape["n"] + 1) // 2
        return {"pairs": _role(pairs, GRAD_WAVES, min(_cdiv(pairs, GRAD_WAVES), cus))}
    raise ValueError(f"unknown op {op}")


def expected_grad_kernels(op, **shape):
    """The demangled kernels one backward call of `op` launches (extra keys of a case are ignored)."""
    if op == "fusion":                                               # mcp_fusion_grad, fusion_grad.hip:474-477
        _fusion(shape["b"], shape["n"], shape.get("nb", 64))
        return {"fusion_grad_kernel", "fusion_grad_reduce_kernel"}
    if op == "cross":
        d = shape["d"]
        _cross(d, shape.get("k", 32))
        if d == 256:                                                 # mcp_cross256_grad's launches, cross256_grad.hip
            return {"cross256_grad_z_kernel", "cross256_grad_w_kernel", "cross256_grad_dx_kernel", "cross256_grad_reduce_kernel"}
        names = {f"cross_grad_kernel<{d}>", "cross_grad_reduce_kernel"}   # launch_cross_grad, cross_grad.hip
        return names | {"transposed_image_kernel"} if d == 128 else names   # !GradShape<D>::WT_LDS, launch_cross_grad
    if op == "pointconv_agg":                                        # pcg_run, pointconv_grad_tile.h; ops.pointconv_agg: d % 4 == 0, d <= 256
        if shape.get("k", 32) != 32 or shape["d"] % 4 or shape["d"] > 256:
            raise ValueError(f"pointconv_agg grad: d={shape['d']} is not built")
        return {"pointconv_agg_grad_kernel", "pointconv_grad_reduce_kernel"}
    if op == "ptblock":                                              # mcp_ptblock_grad, ptblock_grad.hip:456-459
        _ptblock(shape.get("c", 64), shape.get("k", 16))
        return {"ptblock_transposed_images_kernel", "ptblock_grad_kernel", "ptblock_grad_reduce_kernel"}
    raise ValueError(f"unknown op {op}")


def grad_weight_role(case):
    """The role whose rounds decide the layer's largest weight-gradient matrix (the role a dropped or doubled point is looked for in)."""
    if case["op"] == "cross":
        return {64: "all", 128: "own0", 256: "z"}[case["d"]]
    return "points" if case["op"] == "fusion" else "pairs"


GRAD_CASES = [
    # ---- fusion_grad_kernel: one point per wave, 4 waves, grid = min(ceil(total / 4), CUs) ----
    _fus("one-point", 1, 1),                                 # 3 dead waves enter the wave-order sum; every gradient but p2's is zero
    _fus("3-points", 1, 3),                                  # one workgroup, one dead wave
    _fus("5-points", 1, 5),                                  # grid 2, round-robin: the second workgroup has one live wave
    _fus("same-dup", 2, 19, same=True, dup=True, seed=1),    # 38 points, grid 10: zero-length vectors (|r| = 0) and every neighbour twice
    _fus("xcd-ragged", 1, 61),                               # grid 16 by XCD: eighths of 8 points, the last one has 5
    _fus("grid-75", 2, 149, extent=True, seed=4),            # 298 points, grid % 8 = 3: round-robin below the cap, two batch elements
    _fus("cap+1", 5, 205),                                   # 1025 points, want 257 > 256: eighths of 132 against steps of 128, the last has 101: 6 workgroups idle
    _fus("cap-4-rounds", 3, 1031),                           # 3093 points: eighths of 388 = 3 x 128 + 4, the last has 377
    # ---- cross_grad_kernel<64>: one role, grid = min(ceil(total / 4), CUs) ----
    _crs("3-points", 64, 1, 3, 50),                          # one workgroup, one dead wave
    _crs("grid-38", 64, 2, 75, 70),                          # 150 points: round-robin below the cap
    _crs("xcd-ragged", 64, 2, 31, 37, extent=True),          # 62 points, grid 16 by XCD: eighths of 8, the last has 6
    _crs("cap+1", 64, 5, 205, 190),                          # 1025 points: 6 idle workgroups
    _crs("cap-4-rounds", 64, 3, 1031, 900),                  # 3093 points
    # ---- cross_grad_kernel<128>: roles of min(want, CUs / 2) + 2 x min(want, CUs / 4) workgroups, want = ceil(total / 4) ----
    _crs("3-points", 128, 1, 3, 50, seed=1),                 # three workgroups, one per role
    _crs("all-round-robin", 128, 2, 20, 50),                 # 40 points: 10 + 10 + 10
    _crs("xcd-ragged", 128, 3, 127, 150, extent=True),       # 381 points: 96 + 64 + 64 all by XCD, the data role below its cap; eighths of 48, the last has 45
    _crs("base%8", 128, 2, 200, 150),                        # 400 points: 100 + 64 + 64, the data role round-robin and the others too (base 100, 164)
    _crs("cap-3-and-5-rounds", 128, 2, 515, 450),            # 1030 points: 128 + 64 + 64 by XCD, eighths of 132: 3 rounds of 64 (data), 5 of 32; the last has 106
    # ---- cross256_grad_{z,w,dx,reduce}_kernel: z min(ceil(total / 4), 256) round-robin; w min(ceil(total / 8), 64) slices; dx min(total, 512) ----
    _crs("3-points", 256, 1, 3, 50),                         # z: one dead wave; w: one slice; dx: 3 workgroups
    _crs("ragged-workgroup", 256, 3, 83, 70, extent=True),   # 249 points: z grid 63, the last workgroup has one live wave; 32 slices of 8, the last has 1
    _crs("cap+1", 256, 5, 205, 190),                         # 1025 points: z second round for one workgroup; slices of 17: 5 in slice 60, 61..63 empty; dx 3 / 2 points
    _crs("cap-3-rounds", 256, 59, 37, 41),                   # 2183 points: z rounds of 1024 cross 27 batch elements; slices of 35: 13 in the last
    # ---- pointconv_agg_grad_kernel: a wave takes a pair of centres, 4 waves, grid = min(ceil(total / 8), CUs) ----
    _agg("one-centre", 1, 40, 1, 32),                        # the tail alone: the second lane half works on centre 0 with a zero gradient
    _agg("9-centres", 3, 20, 3, 64),                         # 5 pairs, grid 2: the second workgroup has the half pair
    _agg("xcd-ragged-odd", 3, 41, 41, 128),                  # 123 centres, 62 pairs, grid 16 by XCD: eighths of 8 pairs, the last has 6 with the odd tail; S = N
    _agg("cap+1", 3, 700, 683, 32, extent=True),             # 2049 centres, 1025 pairs: 6 idle workgroups, odd tail
    _agg("cap-3-rounds", 3, 1375, 1375, 64),                 # 4125 centres, 2063 pairs: eighths of 260 = 2 x 128 + 4, the last has 243; S = N
    # ---- ptblock_grad_kernel: a wave takes a pair of points, 4 waves, grid = min(ceil(pairs / 4), CUs) ----
    _ptb("one-point", 1, 1),                                 # the odd tail alone
    _ptb("odd-B1", 1, 333, extent=True),                     # 167 pairs, grid 42 round-robin, odd tail
    _ptb("odd-B3", 3, 111, packed=True),                     # 333 points: pairs straddle batch elements; q/k/v with row stride 192
    _ptb("xcd-ragged", 2, 61, logits=80.0),                  # 61 pairs, grid 16 by XCD: eighths of 8, the last has 5; large logits
    _ptb("same-neighbour", 2, 125, same=True),               # a uniform softmax: zero gradients for q and fc_gamma
    _ptb("cap+1", 3, 683),                                   # 2049 points, 1025 pairs: 6 idle workgroups, odd tail
    _ptb("cap-3-rounds", 3, 1375),                           # 4125 points, 2063 pairs
]


# seed: added to the seed the shape gives, where the shape's own data leaves too little of the upstream gradient clear
# (fused_grad_reference.py) or, in grid-75, lets one layer-3 channel win at every neighbour, which makes the gradient of b3 zero


def grad_cases(op):
    return [c for c in GRAD_CASES if c["op"] == op]


# ---- the fusion layer on batch statistics (fusion_bn.hip): one call launches persistent passes under TWO grid caps, every pass deals
# points through mcp_units_by_xcd, and every pass but the layer itself leaves one partial row per workgroup that
# fusion_bn_stats_kernel / sum_partials_kernel add over ALL workgroups ----
BN_WAVES = 4                      # WAVES, fusion_bn.hip:24


def bn_launch_grid(cus=256, **shape):
    """{role: dict(workgroups, units, per, by_xcd, dealt)} of one forward + backward call on a device with `cus` compute units, as
    grad_launch_grid gives it.  "wide": min(ceil(total / 4), 2 CUs) workgroups -- the three statistics passes and the layer (fwd_grid,
    fusion_bn.hip:377-382; the loop :210-211), B1 in both forms and B4 (bwd_grid(total, 2), :1179-1184, :1326, :1351; loops :491-492,
    :631-632, :1065-1066).  "narrow": min(ceil(total / 4), CUs) -- B2 and B3 (bwd_grid(total, 1), :1337, :1344; loops :746-747, :926-927)."""
    total = shape["b"] * shape["n"]
    want = _cdiv(total, BN_WAVES)
    return {"wide": _role(total, BN_WAVES, min(want, 2 * cus)), "narrow": _role(total, BN_WAVES, min(want, cus))}


def expected_bn_kernels(**shape):
    """The demangled kernels that test_fusion_bn_variants_gpu.py launches for a case (extra keys are ignored): the public path
    (be.fusion_bn: mcp_fusion_bn_forward_save, mcp_fusion_bn_backward_saved), the forward that keeps nothing (be.fusion_bn_forward) and,
    unless the case is forward-only, the backward that re-evaluates the layer (mcp_fusion_bn_backward)."""
    if shape.get("nb", 64) != 64:                                    # bn_forward, fusion_bn.hip:1232; bn_backward :1300
        raise ValueError(f"fusion_bn: {shape['nb']} neighbours are not built")
    names = {f"fusion_bn_fwd_kernel<{m}, false>" for m in (1, 2, 3, 0)} | {"fusion_bn_fwd_kernel<0, true>", "fusion_bn_stats_kernel"}   # bn_forward, :1240-1250
    if not shape.get("forward_only"):                                # bn_backward, fusion_bn.hip:1324-1354
        names |= {"transposed_image_kernel", "fusion_bn_b1_saved_kernel", "fusion_bn_b1_kernel", "fusion_bn_b2_kernel", "fusion_bn_b3_kernel",
                  "fusion_bn_b4_kernel", "sum_partials_kernel"}
    return names


def _fbn(tag, b, n, **kw):
    """same / dup / extent / seed as _fus (the data is fused_reference.fusion_inputs'); far: the weights that put the layer-2 conv output
    more than 30 sigma from its bias; forward_only: statistics and out only."""
    return dict(op="fusion_bn", tag=tag, b=b, n=n, **kw)


# at 256 CUs: the wide passes are capped at 512 workgroups, B2 / B3 at 256
BN_CASES = [
    _fbn("one-point", 1, 1),                                 # three dead waves; every channel of every layer has zero variance; every gradient but p2's is zero
    _fbn("3-points", 1, 3),                                  # one workgroup, one dead wave; dead neighbours (no positive layer-3 channel)
    _fbn("5-points", 1, 5),                                  # grid 2 round-robin: the second workgroup has one live wave; dead neighbours
    _fbn("same-dup", 2, 19, same=True, dup=True, seed=1),    # 38 points, grid 10: |r| = 0 and every neighbour twice
    _fbn("xcd-ragged", 1, 61),                               # grid 16 by XCD in every pass: eighths of 8 points, the last has 5
    _fbn("grid-75", 2, 149, extent=True, seed=4),            # 298 points: round-robin below both caps, two batch elements
    _fbn("narrow-cap+1", 5, 205),                            # 1025 points: B2 / B3 want 257 > 256 -- eighths of 132 against steps of 128, the last has 101, 6 idle workgroups; the wide passes: grid 257 round-robin
    _fbn("wide-cap+1", 3, 683),                              # 2049 points: the wide passes want 513 > 512 -- eighths of 260 against steps of 256, the last has 229, 6 idle workgroups, one workgroup per eighth in a second round; B2 / B3: three rounds
    _fbn("cap-rounds", 3, 1031),                             # 3093 points: eighths of 388, the last has 377; two rounds wide, four narrow
    _fbn("far", 2, 149, far=True, forward_only=True),        # the layer-2 conv output sits more than 30 sigma from its bias: statistics and out only
]


def bn_case_id(c):
    shape = ",".join(v if k == "tag" else f"{k}={v}" for k, v in c.items() if k != "op" and v not in (None, False))
    return f"fusion_bn[{shape}]".replace(" ", "")


def grad_case_id(c):
    """A readable pytest id: the backward's main kernel, the tag and the shape."""
    main = sorted(n for n in expected_grad_kernels(**c) if not any(t in n for t in ("reduce", "transposed", "_w_", "_dx_")))[0]
    shape = ",".join(v if k == "tag" else f"{k}={v}" for k, v in c.items() if k != "op" and v not in (None, False))
    return f"{main}[{shape}]".replace(" ", "")


def case_id(c):
    """A readable pytest id: the variant and the shape (the fused cases: their tag first)."""
    shape = ",".join(v if k == "tag" else f"{k}={v}" for k, v in c.items() if k != "op" and v not in (None, False))
    return f"{expected_kernel(**c)}[{shape}]".replace(" ", "")


# ---- the weight gradient of a tall per-point Linear (linear_grad.hip): dW = gz^T x, db = column sums of gz.  A workgroup stages
# 32 rows of both operands, its four waves share the 32 x 32 output tiles, the workgroups' partial results are added by a second kernel ----
WGRAD_ROWS, WGRAD_WAVES, WGRAD_MAX_WGS = 32, 4, 256       # WG_ROWS, WAVES, MAX_WGS, linear_grad.hip:21
WGRAD_MAX_N, WGRAD_MAX_TPW = 256, 16                      # supported(), linear_grad.hip:124; the widest instantiation, :166
WGRAD_LDS_BYTES = 160 * 1024                              # supported(), linear_grad.hip:124; the opt-in, :156
WGRAD_LDS_DEFAULT = 64 * 1024                             # dynamic LDS a kernel may use without the opt-in of :156


def _pad32(v):
    return (v + 31) & ~31                                            # np, kp: linear_grad.hip:33, :123, :147


def wgrad_lds_bytes(n, k):
    return WGRAD_ROWS * (_pad32(n) + _pad32(k) + 8) * 4              # linear_grad.hip:149 (the same expression in supported(), :124)


def wgrad_supported(rows, n, k):
    """supported(), linear_grad.hip:122-125: what mcp_linear_wgrad_workspace_bytes answers with a non-zero size."""
    return (rows > 0 and n > 0 and k > 0 and n <= WGRAD_MAX_N and (_pad32(n) // 32) * (_pad32(k) // 32) <= WGRAD_MAX_TPW * WGRAD_WAVES
            and wgrad_lds_bytes(n, k) <= WGRAD_LDS_BYTES)


def wgrad_max_k(n):
    """The largest k the kernel takes at this n."""
    return max(k for k in range(1, 4096) if wgrad_supported(1, n, k))


def _wgrad_staging(width, stride, offset_floats):
    """(staged as float4, the reasons it is not): linear_grad.hip:45 -- the width a multiple of 32, the row stride a multiple of 4, the
    base on a 16-byte boundary (offset_floats: the view's first element, in floats from its 16-byte-aligned storage)."""
    why = [name for name, bad in (("width", width & 31), ("stride", stride & 3), ("base", (4 * offset_floats) & 15)) if bad]
    return not why, tuple(why)


def wgrad_launch(rows, n, k, gz_stride=None, x_stride=None, gz_offset_floats=0, x_offset_floats=0):
    """The launch mcp_linear_wgrad makes: tiles-per-wave variant, workgroups, stages per workgroup, workgroups left without a stage,
    and how each operand is staged.  Strides default to the widths (contiguous operands)."""
    gs, xs = n if gz_stride is None else gz_stride, k if x_stride is None else x_stride
    if not wgrad_supported(rows, n, k):                              # linear_grad.hip:141
        raise ValueError(f"wgrad: rows={rows}, n={n}, k={k} is not built")
    if gs < n or xs < k:                                             # linear_grad.hip:143
        raise ValueError("wgrad: a row stride below the width")
    stages = _cdiv(rows, WGRAD_ROWS)                                 # linear_grad.hip:146
    wgs = min(stages, WGRAD_MAX_WGS)                                 # wgs_of, linear_grad.hip:126-129
    per = _cdiv(stages, wgs)                                         # linear_grad.hip:146
    tiles = (_pad32(n) // 32) * (_pad32(k) // 32)                    # linear_grad.hip:148
    tpw = _cdiv(tiles, WGRAD_WAVES)
    variant = next(v for v in (1, 2, 4, 8, 16) if tpw <= v)          # linear_grad.hip:162-166
    gz_vec, gz_why = _wgrad_staging(n, gs, gz_offset_floats)
    x_vec, x_why = _wgrad_staging(k, xs, x_offset_floats)
    return dict(variant=variant, kernel=f"linear_wgrad_kernel<{variant}>", workgroups=wgs, stages=stages, stages_per_wg=per,
                idle=wgs - _cdiv(stages, per),                       # workgroup b takes stages b per .. (b + 1) per, linear_grad.hip:44
                tail_rows=rows - (stages - 1) * WGRAD_ROWS,          # live rows of the last stage (the rest are zero-filled, :52, :59)
                tiles=tiles, tiles_per_wave=[len(range(w, tiles, WGRAD_WAVES)) for w in range(WGRAD_WAVES)],   # wave w: tiles w, w + 4, ..., :70
                lds_bytes=wgrad_lds_bytes(n, k), gz_vec=gz_vec, gz_why=gz_why, x_vec=x_vec, x_why=x_why)


def _wg(tag, rows, n, k, gz=None, x=None, block=None):
    """gz / x: None (contiguous), or (W, c0): the operand is columns c0 : c0 + width of a (rows, W) tensor whose other columns hold NaN.
    k = None: the largest k the kernel takes at this n (found by the test through mcp_linear_wgrad_workspace_bytes).
    block = (N, c0): dW / db are rows c0 : c0 + n of an (N, k) / (N,) pair pre-filled with a sentinel (ops._wgrad's column blocks)."""
    return dict(op="wgrad", tag=tag, rows=rows, n=n, k=k, gz=gz, x=x, block=block)


WGRAD_CASES = [
    _wg("one-row", 1, 32, 32),                               # one row, one stage, one partial in the reduce
    _wg("two-stages", 33, 32, 32),                           # two stages, 31 zero-filled rows
    _wg("256-full-stages", 8192, 64, 32),                    # 256 full stages, no tail
    _wg("idle-workgroups", 8193, 3, 32),                     # 257 stages: 2 per workgroup, 127 workgroups idle; n < 32
    _wg("k<32", 2049, 32, 3),                                # element-wise x
    _wg("padded-tiles", 4099, 40, 67),                       # padded tiles both ways: 2 x 3 tiles, variant 2
    _wg("variant-2-whole", 4099, 128, 64),                   # 8 tiles
    _wg("variant-4", 2049, 256, 64),                         # 16 tiles; every thread owns a bias column
    _wg("variant-8-column-block", 2049, 256, 128, gz=(512, 256), block=(512, 256)),   # 32 tiles; ops._wgrad's second column block
    _wg("variant-16-uneven", 4099, 64, 536),                 # 34 tiles: waves 0-1 own nine, waves 2-3 eight (the PointConv projection)
    _wg("variant-16-full", 2049, 256, 256),                  # 64 tiles
    _wg("gz-base", 2049, 64, 64, gz=(68, 1)),                # gz 4 bytes off a 16-byte boundary at a vector width
    _wg("x-stride", 2049, 64, 64, x=(66, 0)),                # x with a row stride that is no multiple of 4
    _wg("gz-stride", 2049, 64, 64, gz=(66, 0)),              # the same two reasons on the other operand
    _wg("x-base", 2049, 64, 64, x=(68, 1)),
    _wg("lds-limit", 2049, 32, None),                        # LDS just under the 160 KB opt-in
]


def wgrad_shape(c):
    """(rows, n, k, gz_stride, x_stride, gz_offset_floats, x_offset_floats) of a case, k = None resolved through the mirror."""
    k = wgrad_max_k(c["n"]) if c["k"] is None else c["k"]
    gs, go = (c["n"], 0) if c["gz"] is None else c["gz"]
    xs, xo = (k, 0) if c["x"] is None else c["x"]
    return c["rows"], c["n"], k, gs, xs, go, xo


def wgrad_case_id(c):
    return f"{wgrad_launch(*wgrad_shape(c))['kernel']}[{c['tag']},rows={c['rows']},n={c['n']},k={c['k'] or 'max'}]"


# ---- the narrow-head attention backward (attention_grad.hip): a wave owns 32 rows of the stationary side (queries in stats and dq,
# keys in dkv), a workgroup 128, the other side streams through double-buffered LDS stages of 64 rows ----
ATTN_GRAD_TILE, ATTN_GRAD_WAVES, ATTN_GRAD_KT = 32, 4, 64     # the MFMA tile; WAVES, KT: attention_grad.hip:19
ATTN_GRAD_BLOCK = ATTN_GRAD_TILE * ATTN_GRAD_WAVES           # rows per workgroup: attention_grad.hip:214, :306, :430, :569
# one row; a wave's tile -1 / 0 / +1; one stage -1 / 0 / +1 (a second stage that holds one row); two stages -1 / 0 / +1 (the third
# stage reuses buffer 0; 128 is also a workgroup block -1 / 0 / +1: a second workgroup that holds one row); 193: the fourth stage reuses buffer 1
ATTN_GRAD_COUNTS = (1, 31, 32, 33, 63, 64, 65, 127, 128, 129, 193)


def attention_small_grad_launch(nq, nk):
    """{kernel: dict(workgroups, last_tile, stages, last_stage)} of one backward call without lengths: `workgroups` along the stationary
    side (launch_all, attention_grad.hip:569), last_tile the live rows of the last wave tile, `stages` of the streamed side
    (:242, :357, :494), last_stage the live rows of the last one."""
    def role(stationary, streamed):
        return dict(workgroups=_cdiv(stationary, ATTN_GRAD_BLOCK), last_tile=(stationary - 1) % ATTN_GRAD_TILE + 1,
                    stages=_cdiv(streamed, ATTN_GRAD_KT), last_stage=(streamed - 1) % ATTN_GRAD_KT + 1)
    return {"attention_stats_kernel": role(nq, nk), "attention_dq_kernel": role(nq, nk), "attention_dkv_kernel": role(nk, nq)}


# ---- the wide-head attention in a training graph (attention_wide_grad.hip; the forward bodies: attention_wide_fwd.h).  Head widths
# 32 / 64: a workgroup is four independent waves of 32 stationary rows each; 256: the four waves share ONE block of 32 rows, each a
# 64-channel slice (GradCfg, attention_wide_grad.hip:77-90).  The other side streams in stages of 32 rows, fetched one stage ahead ----
WIDE_WAVES, WIDE_TILE = 4, 32                                # WAVES, attention_wide_fwd.h:17; the MFMA tile and KT (WideCfg, :33)
WIDE_HEAD_WIDTHS = (32, 64, 256)                             # forward_with / backward_with, attention_wide_grad.hip:416, :439
# one row; a wave's tile -1 / 0 / +1 (33: a second stage that holds one row, and at width 256 a second workgroup that holds one row);
# two stages -1 / 0 / +1 (65: a third stage, which in the query-stationary forward reuses LDS buffer 0, attention_wide_fwd.h:128); 97:
# four stages, each of the forward's two buffers used a second time; 127 / 128 / 129: the 128-row workgroup block of widths 32 / 64 -1 / 0 / +1, and the key-split forward's threshold (four stages,
# one per wave; 129: five, wave 0 takes a second); 161: six stages, waves 0 and 1 take a second
WIDE_GRAD_COUNTS = (1, 31, 32, 33, 63, 64, 65, 97, 127, 128, 129, 161)


def wide_keys_split(bf, nq, nk, heads):
    """wide_keys_split, attention_wide_fwd.h:393-395: read from the padded sizes, never from a length."""
    return _cdiv(nq, WIDE_TILE * WIDE_WAVES) * heads * bf * WIDE_WAVES < 1024 and nk >= WIDE_TILE * WIDE_WAVES


def attention_wide_train_kernels(bf, heads, hd, nq, nk, drop=False, lengths=False):
    """The demangled kernels of one training forward (mcp_attention_wide_lse[_lengths]) plus one backward
    (mcp_attention_wide_grad_lse[_lengths]): launch_forward, attention_wide_grad.hip:55-72; launch_backward :393-410.  drop: drop_p > 0
    (:427, :452); lengths: at least one of the two length arrays is given (:490-491, :499-503)."""
    if hd not in WIDE_HEAD_WIDTHS:
        raise ValueError(f"attention_wide: head width {hd} is not built")
    args = f"{hd}, {'true' if drop else 'false'}" + (", AttnLengths" if lengths else "")
    fwd = "attention_wide_ksplit_lse_kernel" if hd == 256 and wide_keys_split(bf, nq, nk, heads) else "attention_wide_lse_kernel"
    return {f"{fwd}<{args}>", f"attention_wide_dsum_kernel<{hd}>", f"attention_wide_dq_kernel<{args}>", f"attention_wide_dkv_kernel<{args}>"}


def wide_ksplit_waves(keys):
    """Key-split forward: wave w takes the 32-key stages w, w + 4, ... of the element's own key count (attention_wide_fwd.h:294-296)."""
    stages = _cdiv(keys, WIDE_TILE)
    per = [len(range(w, stages, WIDE_WAVES)) for w in range(WIDE_WAVES)]
    return dict(stages_per_wave=per, idle_waves=per.count(0))


def attention_wide_grad_launch(hd, nq, nk, bf=2, heads=2):
    """{kernel: dict(block, workgroups, last_tile, stages, last_stage)} of one training forward + backward without lengths: `block` the
    stationary rows of a workgroup (32 * RPW, GradCfg; the grids: attention_wide_grad.hip:405, :407; the forward's :62, :69),
    `workgroups` along the stationary side, last_tile the live rows of the last 32-row tile, `stages` of the streamed side
    (:215, :333; attention_wide_fwd.h:122, :294), last_stage the live rows of the last one.  The key-split forward adds
    wide_ksplit_waves(nk); attention_wide_dsum_kernel is dict(workgroups, last_block_lanes): rows * hd / 4 lanes in blocks of 256 (:404)."""
    if hd not in WIDE_HEAD_WIDTHS:
        raise ValueError(f"attention_wide: head width {hd} is not built")

    def role(stationary, streamed, block):
        return dict(block=block, workgroups=_cdiv(stationary, block), last_tile=(stationary - 1) % WIDE_TILE + 1,
                    stages=_cdiv(streamed, WIDE_TILE), last_stage=(streamed - 1) % WIDE_TILE + 1)
    block = WIDE_TILE * (1 if hd > 64 else WIDE_WAVES)               # 32 * RPW, RPW = WAVES / SPLIT, SPLIT = HD > 64 ? WAVES : 1
    lanes = bf * nq * heads * (hd // 4)
    out = {"attention_wide_dq_kernel": role(nq, nk, block), "attention_wide_dkv_kernel": role(nk, nq, block),
           "attention_wide_dsum_kernel": dict(workgroups=_cdiv(lanes, 256), last_block_lanes=(lanes - 1) % 256 + 1)}
    if hd == 256 and wide_keys_split(bf, nq, nk, heads):
        out["attention_wide_ksplit_lse_kernel"] = dict(role(nq, nk, WIDE_TILE), **wide_ksplit_waves(nk))
    else:
        out["attention_wide_lse_kernel"] = role(nq, nk, WIDE_TILE * WIDE_WAVES)
    return out


def _wt(kind, hd, nq, nk, bf=2, heads=2, drop=False, qlen=None, klen=None, **kw):
    """kind: guard (canary rows around every output of the C entries), dropout, dropout-lengths, strides (q, k, v slices of one
    (BF, n, 3C) tensor), logits (q scaled by `factor`).  qlen / klen: per-element lengths (None: that side is full)."""
    return dict(kind=kind, bf=bf, heads=heads, hd=hd, nq=nq, nk=nk, drop=drop, qlen=qlen, klen=klen, **kw)


def wide_case_kernels(c):
    return attention_wide_train_kernels(c["bf"], c["heads"], c["hd"], c["nq"], c["nk"], c["drop"], c["qlen"] is not None or c["klen"] is not None)


def wide_case_id(c):
    fwd = "ksplit" if any("ksplit" in n for n in wide_case_kernels(c)) else "qs"
    tail = "".join(f",{k}={'_'.join(map(str, c[k]))}" for k in ("qlen", "klen") if c[k] is not None) + (",drop" if c["drop"] else "")
    return f"{c['kind']}[hd={c['hd']},{c['bf']}x{c['heads']},nq={c['nq']},nk={c['nk']},{fwd}{tail}]"


# section (b): a partial tile on both sides per width, and the key-split forward; each once plain and once through the _lengths entries
# with lengths shorter than the launch
WIDE_GUARD_CASES = [c for hd, nq, nk, heads in ((32, 33, 65, 2), (64, 33, 65, 2), (256, 33, 65, 2), (256, 37, 130, 1))
                    for c in (_wt("guard", hd, nq, nk, heads=heads), _wt("guard", hd, nq, nk, heads=heads, qlen=(nq - 2, 1), klen=(33, nk - 1)))]

WIDE_DROP_SHAPES = ((33, 65), (129, 63), (1, 129), (128, 64))
# (d): 0, 1, 31, 33 and the full count on either side, over three length sets of the two elements
WIDE_LENGTH_SETS = (lambda nq, nk: ((nq, 1), (31, nk)), lambda nq, nk: ((33, 31), (1, 33)), lambda nq, nk: ((0, 33), (nk, 0)))

WIDE_TRAIN_CASES = (
    # (c) dropout at the edges: four shapes per width (at width 256, (1, 129) takes the key-split forward), and two key-split shapes
    # with a partial last stage and unequal stages per wave (130: 5 stages, 2/1/1/1, the last holds 2 keys; 161: 6 stages, 2/2/1/1, 1 key)
    [_wt("dropout", hd, nq, nk, drop=True) for hd in WIDE_HEAD_WIDTHS for nq, nk in WIDE_DROP_SHAPES]
    + [_wt("dropout", 256, 37, nk, heads=1, drop=True) for nk in (130, 161)]
    # (d) dropout with lengths: the query-stationary forward at every width, and the key-split one (a key length <= 32 leaves three
    # waves without a stage, 33 two)
    + [_wt("dropout-lengths", hd, nq, nk, heads=heads, drop=True, qlen=ls(nq, nk)[0], klen=ls(nq, nk)[1])
       for hd, nq, nk, heads in ((32, 130, 100, 2), (64, 130, 100, 2), (256, 130, 100, 2), (256, 37, 130, 1)) for ls in WIDE_LENGTH_SETS]
    # (e) q, k, v with row stride 3C: once per width, and once with dropout and lengths on the key-split forward
    + [_wt("strides", hd, 65, 65) for hd in WIDE_HEAD_WIDTHS]
    + [_wt("strides", 256, 130, 130, heads=1, drop=True, qlen=(33, 130), klen=(130, 31))]
    # (f) large logits on partial tiles
    + [_wt("logits", 256, 33, 65, factor=6.0)]
)


def wide_cases(kind):
    return [c for c in WIDE_TRAIN_CASES if c["kind"] == kind]


# ---- emd_grad.hip: emd_grad_kernel<SIDE, LEN> has 64 lane points per workgroup and streams the other cloud in tiles of 512 of which
# wave w takes entries [64 w, 64 w + 64) (:24, :79-94); matchcost_grad1_kernel gives wave w the w-th eighth of m (:175: empty ranges
# when m < 8), matchcost_grad2_kernel takes 8 rows per workgroup and strides 256 lanes over n (:199-217), matchcost_kernel 1024 (:138-146) ----
EMD_LEAN_SHAPES = ((1, 1), (1, 513), (513, 1), (63, 65), (64, 64), (65, 63), (64, 512), (511, 64), (512, 513), (577, 129))
EMD_MATCH_SHAPES = ((1, 1), (3, 5), (64, 7), (65, 8), (255, 9), (256, 16), (257, 17), (1023, 1), (1024, 3), (1025, 15))
_EMD_PLAIN = ("emd_grad_kernel<1, false>", "emd_grad_kernel<2, false>")
_EMD_LEN = ("emd_grad_kernel<1, true>", "emd_grad_kernel<2, true>")
EMD_GRAD_CASES = (
    [dict(kind="lean", n=n, m=m, len1=None, len2=None, kernels=_EMD_PLAIN) for n, m in EMD_LEAN_SHAPES]
    # mcp_emd_grad_lengths (emd_grad.hip:264-270): full lengths must give the plain call's bits, short ones the sliced call's
    + [dict(kind="lean-lengths", n=n, m=m, len1=(n, n), len2=(m, m), kernels=_EMD_LEN) for n, m in ((63, 65), (512, 513))]
    + [dict(kind="lean-lengths", n=64, m=65, len1=(31, 64), len2=(65, 1), kernels=_EMD_LEN)]
    + [dict(kind="match", n=n, m=m, len1=None, len2=None, kernels=("matchcost_kernel", "matchcost_grad1_kernel", "matchcost_grad2_kernel"))
       for n, m in EMD_MATCH_SHAPES]
)

# ---- interp3_grad.hip: one thread per dense point, 256 per workgroup (:13, :19-20) ----
INTERP3_GRAD_CASES = ([dict(n=n, s=s, coincident=0, kernels=("interp3_weights_grad_kernel",)) for n in (1, 255, 256, 257, 513) for s in (3, 40)]
                      + [dict(n=257, s=40, coincident=5, kernels=("interp3_weights_grad_kernel",))])


def emd_cases(kind):
    return [c for c in EMD_GRAD_CASES if c["kind"] == kind]


# ---- index, blend and normalisation primitives (pointnet2_ops.hip, interp3.hip, norm.hip): the neighbour-row gathers, the scatters
# that carry every coordinate and feature gradient, the 3-NN blend and the Crossformer's normalisation.  Two launch forms: a 1-D
# grid-stride loop whose grid is capped (group_rows and everything channel-last), and one thread per point with the batch element
# (and a chunk of PRIM_CCH channels) on the other grid axes (the channel-major entries of the reference API) ----
MCP_OK, MCP_ERR_BAD_ARG, MCP_ERR_UNSUPPORTED = 0, 10001, 10002   # include/mocopci_hip.h:35-37
PRIM_BLK = 256                                                # BLK, pointnet2_ops.hip:12, interp3.hip:10
PRIM_CCH = 8                                                  # CCH, pointnet2_ops.hip:40
PRIM_SUB = 8                                                  # NARROW_SUB, pointnet2_ops.hip:186; I3_SUB, interp3.hip:88
PRIM_NN_TILE = 1024                                           # NN_TILE, pointnet2_ops.hip:335
PRIM_CAP_8K, PRIM_CAP_16K, PRIM_CAP_MFA = 8192, 16384, 1 << 16
PRIM_LN_ROWS, PRIM_LN_MAX_C = 4, 1024                         # one wave per row, four per workgroup: norm.hip:24, :68; :66
PRIM_LN_PER = (1, 2, 4, 16)                                   # norm.hip:69-72


def _prim_loop(kernel, items, per_wg, cap):
    """A capped grid-stride launch: workgroup w takes items [w per_wg, (w + 1) per_wg) + r grid per_wg of round r."""
    grid = min(_cdiv(min(items, 0x7fffffff), per_wg), cap)
    per_round = grid * per_wg
    rounds = _cdiv(items, per_round)
    last_round = items - (rounds - 1) * per_round
    return dict(kernel=kernel, grid=(grid,), items=items, per_wg=per_wg, cap=cap, rounds=rounds, last_round=last_round,
                last_wg=(last_round - 1) % per_wg + 1)


def _prim_blocks(kernel, points, b, c=None):
    """One thread per point, PRIM_BLK per workgroup, no loop; c: the kernel walks chunks of PRIM_CCH channels on blockIdx.y."""
    grid = (_cdiv(points, PRIM_BLK), b) if c is None else (_cdiv(points, PRIM_BLK), _cdiv(c, PRIM_CCH), b)
    out = dict(kernel=kernel, grid=grid, items=points, per_wg=PRIM_BLK, cap=None, rounds=1, last_round=points,
               last_wg=(points - 1) % PRIM_BLK + 1)
    if c is not None:
        out["last_chunk"] = (c - 1) % PRIM_CCH + 1
    return out


# which operands each entry tests for a 16-byte base (the route it takes when one is off: "scalar" twin or MCP_ERR_BAD_ARG)
PRIM_ALIGNED_OPERANDS = {
    "mcp_group_rows": ("points", "out"),                                   # pointnet2_ops.hip:475
    "mcp_group_rows_add_leaky": ("points", "centre", "out"),               # :494
    "mcp_group_rows_grad_sorted": ("grad_out", "grad_points"),             # :523
    "mcp_interp3_apply": ("feat", "out"),                                  # interp3.hip:193
    "mcp_interp3_apply_grad_sorted": ("grad_out", "feat", "grad_feat"),    # interp3.hip:161 (grad_w3), :168 (grad_feat)
    "mcp_mfa_prepare": ("fea", "te_self", "te_partner", "scale", "shift", "x", "xn", "xr"),   # norm.hip:108
}


def primitive_launch(entry, aligned=True, off=None, **s):
    """dict(status, launches) of one call of a C entry of the three units: the status the host returns (no launch unless MCP_OK) and, per
    kernel in launch order, dict(kernel, grid, items, per_wg, cap, rounds = ceil(items / (grid x per_wg)), last_round = live items of
    the last round, last_wg = live items of its last live workgroup), plus last_chunk (channels of the last blockIdx.y), tiles /
    last_tile (three_nn) and registers / last_register (add_layernorm) where the kernel has them.  aligned=False: every operand the
    host tests (PRIM_ALIGNED_OPERANDS) is off a 16-byte boundary; off=(names): only those.  Shape keywords are the C arguments."""
    tested = PRIM_ALIGNED_OPERANDS.get(entry, ())
    bad = set(tested if off is None and not aligned else off or ())
    if bad - set(tested):
        raise ValueError(f"{entry} does not test the alignment of {sorted(bad - set(tested))}")

    def al(*names):
        return not bad & set(names)

    def ok(*launches):
        return dict(status=MCP_OK, launches=list(launches))

    def err(status):
        return dict(status=status, launches=[])
    if any(v <= 0 for k, v in s.items() if k not in ("want", "x_stride", "y_stride", "out_stride", "with_y")):
        return err(MCP_ERR_BAD_ARG)                                         # MCP_CHECK_ARGS of every entry
    g = s.get
    if entry == "mcp_gather_points":                                        # pointnet2_ops.hip:424
        return ok(_prim_blocks("gather_points_kernel", g("npoints"), g("b")))
    if entry == "mcp_gather_points_grad":                                   # :432
        return ok(_prim_blocks("gather_points_grad_kernel", g("npoints"), g("b")))
    if entry == "mcp_group_points":                                         # :440-441
        return ok(_prim_blocks("group_points_kernel", g("npoints") * g("nsample"), g("b"), g("c")))
    if entry == "mcp_group_points_grad":                                    # :449-450
        return ok(_prim_blocks("group_points_grad_kernel", g("npoints") * g("nsample"), g("b"), g("c")))
    if entry == "mcp_group_points_grad_sorted":                             # :458: one thread per DESTINATION n
        return ok(_prim_blocks("scatter_cm_sorted_kernel<false>", g("n"), g("b"), g("c")))
    if entry == "mcp_three_interpolate_grad_sorted":                        # :466: destinations m
        return ok(_prim_blocks("scatter_cm_sorted_kernel<true>", g("m"), g("b"), g("c")))
    if entry == "mcp_three_interpolate":                                    # :585
        return ok(_prim_blocks("three_interpolate_kernel", g("n"), g("b"), g("c")))
    if entry == "mcp_three_interpolate_grad":                               # :593
        return ok(_prim_blocks("three_interpolate_grad_kernel", g("n"), g("b"), g("c")))
    if entry == "mcp_three_nn":                                             # :577; the tile walk :350-351
        out = _prim_blocks("three_nn_kernel", g("n"), g("b"))
        out.update(tiles=_cdiv(g("m"), PRIM_NN_TILE), last_tile=(g("m") - 1) % PRIM_NN_TILE + 1)
        return ok(out)
    if entry == "mcp_group_rows":                                           # :475-486
        b, c, t = g("b"), g("c"), g("t")
        if c % 4 == 0 and al("points", "out"):
            return ok(_prim_loop("group_rows_kernel<HIP_vector_type<float, 4u>, 4>", b * t * (c // 4), PRIM_BLK, PRIM_CAP_8K))
        return ok(_prim_loop("group_rows_kernel<float, 1>", b * t * c, PRIM_BLK, PRIM_CAP_8K))
    if entry == "mcp_group_rows_add_leaky":                                 # :494-498
        if g("c") % 4 or not al("points", "centre", "out"):
            return err(MCP_ERR_BAD_ARG)
        return ok(_prim_loop("group_rows_add_leaky_kernel", g("b") * g("s") * g("k") * (g("c") // 4), PRIM_BLK, PRIM_CAP_16K))
    if entry == "mcp_group_rows_grad":                                      # :507-509
        return ok(_prim_loop("group_rows_grad_kernel", g("b") * g("t") * g("c"), PRIM_BLK, PRIM_CAP_8K))
    if entry == "mcp_group_rows_grad_sorted":                               # :516-531
        b, n, c = g("b"), g("n"), g("c")
        if c <= 4:                                                          # :516-518: NARROW_SUB lanes per row, whatever the alignment
            return ok(_prim_loop("group_rows_grad_sorted_narrow_kernel", b * n, PRIM_BLK // PRIM_SUB, PRIM_CAP_16K))
        vec4 = c % 4 == 0 and al("grad_out", "grad_points")                 # :523
        return ok(_prim_loop(f"group_rows_grad_sorted_kernel<{'true' if vec4 else 'false'}>", b * n * (c // 4 if vec4 else c),
                             PRIM_BLK, PRIM_CAP_16K))
    if entry == "mcp_interp3_apply":                                        # interp3.hip:193-204
        b, n, c = g("b"), g("n"), g("c")
        if c % 4 == 0 and al("feat", "out"):
            return ok(_prim_loop("interp3_apply_kernel<HIP_vector_type<float, 4u>, 4>", b * n * (c // 4), PRIM_BLK, PRIM_CAP_8K))
        return ok(_prim_loop("interp3_apply_kernel<float, 1>", b * n * c, PRIM_BLK, PRIM_CAP_8K))
    if entry == "mcp_interp3_apply_grad":                                   # interp3.hip:182-183
        return ok(_prim_loop("interp3_apply_grad_kernel", g("b") * g("n") * g("c"), PRIM_BLK, PRIM_CAP_8K))
    if entry == "mcp_interp3_apply_grad_sorted":                            # interp3.hip:155-176
        b, n, sp, c, want = g("b"), g("n"), g("s"), g("c"), g("want", ("feat", "w"))
        if not want:
            return err(MCP_ERR_BAD_ARG)                                     # :155
        launches = []
        if "w" in want:                                                     # :160-163: I3_SUB lanes per (point, neighbour)
            w = _prim_loop("interp3_grad_w_kernel", b * n * 3, PRIM_BLK // PRIM_SUB, PRIM_CAP_16K)
            w["vec"] = int(c % 4 == 0 and al("grad_out", "feat"))
            w["passes"] = _cdiv(c // 4 if w["vec"] else c, PRIM_SUB)        # :101, :106: strides of I3_SUB lanes over the row
            launches.append(w)
        if "feat" in want:                                                  # :168-174
            vec4 = c % 4 == 0 and al("grad_out", "grad_feat")
            launches.append(_prim_loop(f"interp3_grad_feat_sorted_kernel<{'true' if vec4 else 'false'}>", b * sp * (c // 4 if vec4 else c),
                                       PRIM_BLK, PRIM_CAP_16K))
        return ok(*launches)
    if entry == "mcp_interp3_weights":                                      # interp3.hip:211
        return ok(_prim_blocks("interp3_weights_kernel", g("n"), g("b")))
    if entry == "mcp_interp3":                                              # interp3.hip:221-223: the search (knn.hip) is not mirrored here
        return ok(_prim_blocks("interp3_weights_kernel", g("n"), g("b")), *primitive_launch("mcp_interp3_apply", aligned, off, **s)["launches"])
    if entry == "mcp_add_layernorm":                                        # norm.hip:65-72
        rows, c = g("rows"), g("c")
        if g("x_stride", c) < c or g("out_stride", c) < c or (g("with_y", True) and g("y_stride", c) < c):
            return err(MCP_ERR_BAD_ARG)                                     # :65
        if c > PRIM_LN_MAX_C:
            return err(MCP_ERR_UNSUPPORTED)                                 # :66
        per = next(p for p in PRIM_LN_PER if c <= 64 * p)                   # :69-72
        return ok(dict(kernel=f"add_layernorm_kernel<{per}>", grid=(_cdiv(rows, PRIM_LN_ROWS),), items=rows, per_wg=PRIM_LN_ROWS, cap=None,
                       rounds=1, last_round=rows, last_wg=(rows - 1) % PRIM_LN_ROWS + 1,      # live waves of the last workgroup, :24-25
                       per=per, registers=_cdiv(c, 64), last_register=(c - 1) % 64 + 1))       # live lanes of the last live register, :30-32
    if entry == "mcp_mfa_prepare":                                          # norm.hip:107-113
        if g("c") & 3:
            return err(MCP_ERR_UNSUPPORTED)                                 # :107
        if bad:
            return err(MCP_ERR_BAD_ARG)                                     # :108-110
        return ok(_prim_loop("mfa_prepare_kernel", g("rows") * g("n") * (g("c") // 4), 256, PRIM_CAP_MFA))
    raise ValueError(f"{entry}: not an entry of the index, blend and normalisation units")


def _pc(entry, edge, off=(), **kw):
    """One case.  shape: the C arguments; off: operands placed 4 bytes past a 16-byte boundary; every other keyword is read by the test
    of that entry (src: rows / points gathered from, data="real": random reals against the C oracle, segments="ops": (order, seg) from
    ops._scatter_segments, grid: coordinates on a half-unit grid, coincident: dense points on sparse points)."""
    extras = {k: kw.pop(k) for k in ("data", "segments", "grid", "coincident", "twice") if k in kw}
    launch = primitive_launch(entry, aligned=not off, off=off, **kw)
    return dict(entry=entry, shape=kw, off=tuple(off), status=launch["status"], kernels=tuple(l["kernel"] for l in launch["launches"]),
                edge=edge, **extras)


PRIM_PAST_8K_VEC = dict(b=3, t=10923, c=256)      # 2 097 216 float4 items: 64 past 8192 x 256
PRIM_PAST_8K_SCALAR = dict(b=3, t=19973, c=35)    # 2 097 165 items: 13 past
# thread-axis count x channels of the channel-major entries: every count and every c once, and (257, 9) together
PRIM_CM_PAIRS = ((1, 1), (255, 7), (256, 8), (257, 9), (255, 17))
_CM_SPLIT = {1: (1, 1), 255: (85, 3), 256: (32, 8), 257: (257, 1)}     # group_points: npoints x nsample

PRIMITIVE_CASES = (
    # -- channel-major entries: BLK -1 / 0 / +1 on the thread axis, CCH -1 / 0 / +1 and the third chunk's first channel on blockIdx.y --
    [_pc(e, f"points={p},c={c}", b=3, c=c, n=37, npoints=p, **({"data": "real"} if (p, c) == (257, 9) and not e.endswith("grad") else {}))
     for e in ("mcp_gather_points", "mcp_gather_points_grad") for p, c in PRIM_CM_PAIRS]
    + [_pc(e, f"points={p},c={c}", b=3, c=c, n=37, npoints=_CM_SPLIT[p][0], nsample=_CM_SPLIT[p][1],
           **({"data": "real"} if (p, c) == (257, 9) and not e.endswith("grad") else {}))
       for e in ("mcp_group_points", "mcp_group_points_grad") for p, c in PRIM_CM_PAIRS]
    + [_pc(e, f"points={p},c={c}", b=3, c=c, m=37, n=p, **({"data": "real"} if (p, c) == (257, 9) and not e.endswith("grad") else {}))
       for e in ("mcp_three_interpolate", "mcp_three_interpolate_grad") for p, c in PRIM_CM_PAIRS]
    + [_pc("mcp_group_points_grad_sorted", f"destinations={p},c={c}", b=3, c=c, n=p, t=700) for p, c in PRIM_CM_PAIRS]
    + [_pc("mcp_group_points_grad_sorted", "the oracle's loop on real data", b=3, c=9, n=257, t=700, data="real"),
       _pc("mcp_group_points_grad_sorted", "segments from ops._scatter_segments", b=3, c=9, n=257, t=700, segments="ops")]
    + [_pc("mcp_three_interpolate_grad_sorted", f"destinations={p},c={c}", b=3, c=c, n=233, m=p) for p, c in PRIM_CM_PAIRS]
    + [_pc("mcp_three_interpolate_grad_sorted", "the oracle's loop on real data", b=3, c=9, n=233, m=257, data="real"),
       _pc("mcp_three_interpolate_grad_sorted", "segments from ops._scatter_segments", b=3, c=9, n=233, m=257, segments="ops")]
    # -- group_rows / interp3_apply: both routes, both reasons for the scalar one, one item, a second round of a few items --
    + [_pc("mcp_group_rows", "one item", b=1, n=1, c=1, t=1)]
    + [_pc("mcp_group_rows", f"c={c}", b=3, n=50, c=c, t=70) for c in (1, 3, 4, 5, 256)]
    + [_pc("mcp_group_rows", f"c=64, {o} off 16 bytes", off=(o,), b=3, n=50, c=64, t=70) for o in ("points", "out")]
    + [_pc("mcp_group_rows", "second round, float4", n=50, twice=True, **PRIM_PAST_8K_VEC),
       _pc("mcp_group_rows", "second round, scalar", n=50, twice=True, **PRIM_PAST_8K_SCALAR)]
    + [_pc("mcp_interp3_apply", "one item", b=1, n=1, s=3, c=1)]
    + [_pc("mcp_interp3_apply", f"c={c}", b=3, n=70, s=50, c=c) for c in (1, 3, 4, 5, 256)]
    + [_pc("mcp_interp3_apply", f"c=64, {o} off 16 bytes", off=(o,), b=3, n=70, s=50, c=64) for o in ("feat", "out")]
    + [_pc("mcp_interp3_apply", "second round, float4", b=3, n=10923, s=50, c=256, twice=True),
       _pc("mcp_interp3_apply", "second round, scalar", b=3, n=19973, s=50, c=35, twice=True)]
    # -- group_rows_add_leaky: float4 only; the refusals --
    + [_pc("mcp_group_rows_add_leaky", f"c={c}", b=3, n=40, c=c, s=7, k=5) for c in (4, 24, 256)]
    + [_pc("mcp_group_rows_add_leaky", "second round", b=1, n=50, c=256, s=8193, k=8, twice=True),
       _pc("mcp_group_rows_add_leaky", "c % 4 != 0 is refused", b=3, n=40, c=6, s=7, k=5)]
    + [_pc("mcp_group_rows_add_leaky", f"{o} off 16 bytes is refused", off=(o,), b=3, n=40, c=64, s=7, k=5) for o in ("points", "centre", "out")]
    # -- group_rows_grad_sorted: the narrow kernel, both wide ones, both reasons for <false>, a second round of each --
    + [_pc("mcp_group_rows_grad_sorted", f"narrow c={c}", b=3, n=61, c=c, t=2300) for c in (1, 2, 3, 4)]
    + [_pc("mcp_group_rows_grad_sorted", f"c={c}", b=3, n=61, c=c, t=2300) for c in (5, 8, 35, 256)]
    + [_pc("mcp_group_rows_grad_sorted", f"c=64, {o} off 16 bytes", off=(o,), b=3, n=61, c=64, t=2300) for o in ("grad_out", "grad_points")]
    + [_pc("mcp_group_rows_grad_sorted", "narrow, off 16 bytes: still the narrow kernel", off=("grad_out", "grad_points"), b=3, n=61, c=4, t=2300),
       _pc("mcp_group_rows_grad_sorted", "segments from ops._scatter_segments", b=3, n=61, c=8, t=2300, segments="ops"),
       _pc("mcp_group_rows_grad_sorted", "narrow, segments from ops._scatter_segments", b=3, n=61, c=3, t=2300, segments="ops"),
       _pc("mcp_group_rows_grad_sorted", "second round, <true>", b=3, n=21846, c=256, t=2300, twice=True),
       _pc("mcp_group_rows_grad_sorted", "second round, <false>", b=3, n=39946, c=35, t=2300, twice=True),
       _pc("mcp_group_rows_grad_sorted", "second round, narrow", b=1, n=524289 + 5, c=3, t=2300, twice=True)]
    # -- interp3_apply_grad_sorted: both kernels, each alone, vec by c % 4 and by alignment, lane strides below / at / above one pass --
    + [_pc("mcp_interp3_apply_grad_sorted", f"c={c}", b=3, n=70, s=50, c=c) for c in (1, 4, 28, 32, 36)]
    + [_pc("mcp_interp3_apply_grad_sorted", f"c=32, {'grad_' + w if w == 'feat' else 'grad_w3'} alone", b=3, n=70, s=50, c=32, want=(w,)) for w in ("feat", "w")]
    + [_pc("mcp_interp3_apply_grad_sorted", f"c=64, {o} off 16 bytes", off=(o,), b=3, n=70, s=50, c=64) for o in ("grad_out", "feat", "grad_feat")]
    + [_pc("mcp_interp3_apply_grad_sorted", "segments from ops._scatter_segments", b=3, n=70, s=50, c=32, segments="ops"),
       _pc("mcp_interp3_apply_grad_sorted", "second round of grad_feat, <true>", b=3, n=700, s=21846, c=256, twice=True),
       _pc("mcp_interp3_apply_grad_sorted", "second round of grad_feat, <false>", b=3, n=700, s=39946, c=35, twice=True),
       _pc("mcp_interp3_apply_grad_sorted", "second round of grad_w3", b=1, n=174764 + 3, s=50, c=8, twice=True)]
    # -- the atomic scatters of the public ABI --
    + [_pc("mcp_group_rows_grad", f"c={c}", b=3, n=50, c=c, t=70) for c in (1, 3, 4, 5, 256)]
    + [_pc("mcp_group_rows_grad", "second round", n=50, **PRIM_PAST_8K_SCALAR)]
    + [_pc("mcp_interp3_apply_grad", f"c={c}", b=3, n=70, s=50, c=c) for c in (1, 3, 4, 5, 256)]
    + [_pc("mcp_interp3_apply_grad", "second round", b=3, n=19973, s=50, c=35)]
    # -- three_nn: fewer known points than neighbours, NN_TILE -1 / 0 / +1, a third tile of one point; BLK -1 / 0 / +1 unknown points --
    + [_pc("mcp_three_nn", f"n={n},m={m}", b=3, n=n, m=m) for n, m in ((1, 1), (255, 2), (256, 3), (257, 4), (1, 1023), (255, 1024), (256, 1025), (257, 2049))]
    + [_pc("mcp_three_nn", "ties across the tile boundaries", b=3, n=257, m=2049, grid=True)]
    # -- interp3 / interp3_weights --
    + [_pc("mcp_interp3", f"n={n},s={sp}", b=3, n=n, s=sp, c=c) for n, c in ((1, 5), (255, 8), (256, 5), (257, 8)) for sp in (3, 40)]
    + [_pc("mcp_interp3", "dense points on sparse points: the 1e-10 clamp", b=3, n=257, s=40, c=8, coincident=5)]
    + [_pc("mcp_interp3_weights", f"n={n},s={sp}", b=3, n=n, s=sp) for n in (1, 255, 256, 257) for sp in (3, 40)]
    + [_pc("mcp_interp3_weights", "dense points on sparse points: the 1e-10 clamp", b=3, n=257, s=40, coincident=5)]
    # -- add_layernorm: every register boundary of every PER at five rows (one live wave in the second workgroup), every row count at c = 65 --
    + [_pc("mcp_add_layernorm", f"rows=5,c={c}", rows=5, c=c) for c in (1, 63, 64, 65, 127, 128, 129, 255, 256, 257, 1023, 1024)]
    + [_pc("mcp_add_layernorm", f"rows={r},c=65", rows=r, c=65) for r in (1, 2, 3, 4, 1027)]
    + [_pc("mcp_add_layernorm", f"rows=1027,c={c}", rows=1027, c=c) for c in (64, 256, 1024)]
    + [_pc("mcp_add_layernorm", "c = 1025 is unsupported", rows=5, c=1025),
       _pc("mcp_add_layernorm", "a stride below c is refused", rows=5, c=65, x_stride=64)]
    # -- mfa_prepare --
    + [_pc("mcp_mfa_prepare", f"rows={r},n={n},c={c}", rows=r, n=n, c=c) for r, n, c in ((1, 1, 4), (5, 33, 64), (1, 33, 64), (5, 1, 4))]
    + [_pc("mcp_mfa_prepare", "c = 6 is unsupported", rows=5, n=33, c=6)]
    + [_pc("mcp_mfa_prepare", f"{o} off 16 bytes is refused", off=(o,), rows=5, n=33, c=64) for o in PRIM_ALIGNED_OPERANDS["mcp_mfa_prepare"]]
)


def primitive_cases(entry, ok=None):
    """The cases of one entry; ok=True / False: only those the host accepts / refuses."""
    return [c for c in PRIMITIVE_CASES if c["entry"] == entry and (ok is None or (c["status"] == MCP_OK) == ok)]


def primitive_case_launch(c):
    return primitive_launch(c["entry"], aligned=not c["off"], off=c["off"], **c["shape"])


def primitive_case_id(c):
    shape = ",".join(f"{k}={'+'.join(v) if isinstance(v, tuple) else v}" for k, v in c["shape"].items())
    tail = "".join(f",{k}" for k in ("data", "segments", "grid", "coincident") if c.get(k)) + ("".join(f",{o}+4B" for o in c["off"]))
    return f"{c['entry'][4:]}[{shape}{tail}]"
