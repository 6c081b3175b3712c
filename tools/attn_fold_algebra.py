import torch
torch.manual_seed(0)
def run(C, Lq, Lk=18, heads=2, n=4):
    d = C // heads
    g = torch.Generator().manual_seed(C)
    r = lambda *s, sc=1.0: (torch.randn(*s, generator=g, dtype=torch.float64) * sc)
    qin, kp, vp, x = r(n, Lq, C), r(n, Lk, C), r(n, Lk, C), r(n, Lq, C)
    Wq, Wk, Wv, Wp = (r(C, C, sc=C ** -0.5) for _ in range(4))
    bq, bk, bv, bp = (r(C, sc=0.1) for _ in range(4))
    scale = C ** -0.5
    def ref(dt):
        c = lambda t: t.to(dt)
        q = c(qin) @ c(Wq).T + c(bq); k = c(kp) @ c(Wk).T + c(bk); v = c(vp) @ c(Wv).T + c(bv)
        qh, kh, vh = (t.reshape(n, -1, heads, d).transpose(1, 2) for t in (q, k, v))
        o = (torch.softmax(qh @ kh.transpose(-1, -2) * scale, -1) @ vh).transpose(1, 2).reshape(n, Lq, C)
        return o @ c(Wp).T + c(bp) + c(x)
    def folded(dt):
        # weight-only folds in fp64, stored in dt (done once per parameter version)
        out = None
        c = lambda t: t.to(dt)
        acc = c(x) + c(bp + Wp @ bv)
        for h in range(heads):
            s = slice(h * d, (h + 1) * d)
            Wkq = c(Wk[s].T @ Wq[s])            # [C_in(k), C_in(q)]
            ukq = c(Wk[s].T @ bq[s])            # [C]
            Wvp = c(Wv[s].T @ Wp[:, s].T)       # [C_in(v), C_out]
            G = c(kp) @ Wkq                     # [n, Lk, C]
            s0 = c(kp) @ ukq                    # [n, Lk]
            U = c(vp) @ Wvp                     # [n, Lk, C]
            S = (c(qin) @ G.transpose(-1, -2) + s0[:, None, :]) * scale
            acc = acc + torch.softmax(S, -1) @ U
        return acc
    r64 = ref(torch.float64)
    e_ref = (ref(torch.float32).double() - r64).abs().max().item() / r64.abs().max().item()
    e_fold = (folded(torch.float32).double() - r64).abs().max().item() / r64.abs().max().item()
    e_alg = (folded(torch.float64) - r64).abs().max().item() / r64.abs().max().item()
    print(f"C={C} Lq={Lq}: fp32 reference-order err {e_ref:.2e}, fp32 folded err {e_fold:.2e}, fp64 folded-vs-ref {e_alg:.2e}")
for C, Lq in ((768, 84), (384, 336), (192, 1344), (96, 5376)):
    run(C, Lq)
