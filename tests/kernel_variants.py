"""The dense-layer kernel variants (csrc/linear.hip, mlp.hip, attention.hip) and the parity cases that reach them.

expected_kernel() mirrors the C dispatch: given an entry point and a shape it names the template instantiation that runs, in
the form c++filt prints it without namespace and arguments ("linear_kernel<3, 2, 8>").  CASES parametrises
test_kernel_variants_gpu.py; test_kernel_variants_cpu.py checks that every instantiation in the device assembly is named by at
least one case, so a variant added later without a parity case fails the CPU suite.  A plain module, imported by both tests."""


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
    if hd in (8, 16):                                                # attention_any, attention.hip:532-538
        return f"attention_small_kernel<{hd}>"
    if hd in (32, 64):                                               # attention.hip:541-542
        return f"attention_wide_kernel<{hd}>"
    if hd == 256:                                                    # attention.hip:545-547
        if _cdiv(nq, 128) * heads * bf * 4 < 1024 and nk >= 128:
            return "attention_wide_ksplit_kernel<256>"
        return "attention_wide_kernel<256>"
    raise ValueError(f"attention: head width {hd} is not built")      # mcp_attention, attention.hip:574


def expected_kernel(op, **shape):
    """Demangled name of the kernel the entry point `op` launches for `shape` (extra keys of a case are ignored):
    linear (rows, ks, n[, policy_rows]), linear_narrow (k, n), mlp2 (rows, cin, hidden, cout), attention (bf, nq, nk, heads, hd)."""
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
]


def cases(op):
    return [c for c in CASES if c["op"] == op]


def case_id(c):
    """A readable pytest id: the variant and the shape."""
    shape = ",".join(f"{k}={v}" for k, v in c.items() if k != "op" and v not in (None, False))
    return f"{expected_kernel(**c)}[{shape}]".replace(" ", "")
