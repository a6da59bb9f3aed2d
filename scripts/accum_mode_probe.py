#!/usr/bin/env python3
"""Scheme-1 accumulator with a surface frame every 33 slices: the event-pixel update (dense=False) against the every-pixel
pass (dense=True: groups of 64 slices) at 1280x720 and 3840x2160 -- which one the automatic mode should take."""
import sys, time
import os
_root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [_root, os.path.join(_root, "neuromorphic-spatiotemporal-optical-flow_amd")]
os.environ.setdefault("NSOF_SKIP_BUILD","1")
import torch, nsof
from nsof import synth
from nsof.accumulator import Accumulator, slice_index_array
ctx = nsof.Context(0); dev = torch.device("cuda",0)
for (H,W,nbg) in [(720,1280,200_000),(720,1280,5_000),(2160,3840,None)]:
    if nbg is None: x,y,p,t = synth.make_event_stream_4k()
    else: x,y,p,t = synth.make_events(2024, W, H, n_background=nbg)
    idx = slice_index_array(t, 1000); every=33; nf=(len(idx)-1)//every
    frames = torch.empty((nf,H,W),dtype=torch.uint8,device=dev); torch.cuda.synchronize()
    for dense in (False, True):
        acc = Accumulator(H,W,1,"split",-6.0,0.0,ctx=ctx,dense=dense); acc.set_events(x,y,p,t,idx)
        best=1e9
        for rep in range(4):
            acc.reset(); ctx.synchronize(); t0=time.perf_counter()
            acc.run_frames(0,nf,every,frames); ctx.synchronize(); best=min(best,time.perf_counter()-t0)
        print(f"{W}x{H} bg={nbg} dense={dense}: {best*1e3:.3f} ms for {nf} frames ({nf*every/best:.0f} slices/s) checksum {int(frames.to(torch.int64).sum().item())}", flush=True)
        acc.close()
