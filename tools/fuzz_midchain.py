"""Fuzz: small-minibatch steps on the two cooperative launches of midchain.hip against the
chain of launches over random shapes (rows x samples <= 128, widths <= 128, 1-3 layers, all
four count likelihoods): every scalar, the per-cell log-likelihood, each gradient, moving
statistic and parameter tensor by name, and an evaluation step's scalars, each within 5e-5 of
its own magnitude.  A non-finite value on either side is a mismatch.  Each step asserts the
path it took (``Engine.uses_mid_chain``).
Usage (GPU box): PYTHONPATH=. python tools/fuzz_midchain.py <seed> <configs>"""
import numpy as np, torch, sys
from scvae_amd.engine import Engine
dev=torch.device("cuda:0")
rng=np.random.default_rng(int(sys.argv[1]) if len(sys.argv)>1 else 0)
bad=0; n=0
LK=["negative binomial","poisson","zero-inflated negative binomial","zero-inflated poisson"]

def tensors(eng, s, ll, ev):
    """name -> flat host tensor: scalars one by one, the state buffers per named tensor."""
    out={}
    for i in range(s.numel()): out["scalar %d"%i]=s[i:i+1]
    out["log_p_x_given_z"]=ll
    for kind,flat,table in (("grad",eng.grads,eng.param_table),("moving",eng.moving,eng.moving_table),
                            ("param",eng.params,eng.param_table)):
        flat=flat.clone().cpu()
        for name,(off,shape) in table.items():
            out[kind+" "+name]=flat[off:off+int(np.prod(shape))]
    for i in range(ev.numel()): out["eval scalar %d"%i]=ev[i:i+1]
    return out

for it in range(int(sys.argv[2]) if len(sys.argv)>2 else 150):
    n_iw=int(rng.integers(1,4)); n_mc=int(rng.integers(1,3))
    S=n_iw*n_mc
    B=int(rng.integers(1,128//S+1))
    nl=int(rng.integers(1,4))
    H=tuple(int(rng.integers(1,129)) for _ in range(nl))
    L=int(rng.integers(1,129))
    F=int(rng.integers(5,400))
    lk=LK[int(rng.integers(0,4))]
    x=torch.from_numpy((rng.poisson(2.,(B,F))*(rng.random((B,F))<0.3)).astype(np.float32)).to(dev)
    eps=torch.from_numpy(rng.standard_normal((S,B,L)).astype(np.float32)).to(dev)
    res=[]
    try:
        for mid in (True,False):
            eng=Engine(F,L,H,lk,batch_norm=True,device=dev,seed=3)
            g=torch.Generator().manual_seed(9)
            for name,p in eng.named_parameters().items():
                if not name.endswith("weights"): p.copy_(torch.randn(p.shape,generator=g)*0.1)
            eng.set_mid_chain(mid)
            eng.reserve(B,S)
            assert eng.uses_mid_chain(B,S)==mid and eng.uses_mid_chain(B,S,training=False)==mid
            ll=torch.zeros(S*B,device=dev)
            s=eng.step(x,x,eps=eps,training=True,n_iw=n_iw,n_mc=n_mc,warm_up_weight=0.6,outputs={"log_p_x_given_z":ll}).clone()
            ev=eng.step(x,x,eps=eps,training=False,n_iw=n_iw,n_mc=n_mc).clone()
            torch.cuda.synchronize()
            res.append(tensors(eng,s.cpu(),ll.cpu(),ev.cpu()))
    except Exception as e:
        print("EXC",B,H,L,F,lk,n_iw,n_mc,repr(e)[:200]); bad+=1; continue
    n+=1
    a,b=res
    for name in b:
        u,v=a[name].double(),b[name].double()
        if not (torch.isfinite(u).all() and torch.isfinite(v).all()):
            print("NONFINITE",name,B,H,L,F,lk,n_iw,n_mc); bad+=1; break
        if v.numel()==0: continue
        sc=v.abs().max().item()
        err=(u-v).abs().max().item()
        if err>5e-5*sc+1e-8:
            print("MISMATCH",name,err/(sc+1e-30),B,H,L,F,lk,n_iw,n_mc); bad+=1; break
print("configs",n,"bad",bad)
