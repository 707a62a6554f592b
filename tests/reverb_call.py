"""sir_wave_reverb_mix through its C entry point with raw tensors, for the GPU tests of the stage: they control strides, fills
and bad arguments themselves."""
import numpy as np
import torch

from sir_amd import _native

NAN = float("nan")


def bank(rows, fill=0.0, extra=8):
    """[n][stride] float32 on the GPU with `fill` behind each row's length, and the lengths"""
    n = max(len(r) for r in rows)
    t = torch.full((len(rows), (n + 7) // 8 * 8 + extra), fill, dtype=torch.float32)
    for i, r in enumerate(rows):
        t[i, :len(r)] = torch.as_tensor(r)
    return t.cuda(), torch.tensor([len(r) for r in rows], dtype=torch.int32).cuda()


def i32(v):
    return None if v is None else torch.tensor(v, dtype=torch.int32).cuda()


def call(fz, wave, lengths, rir=None, rir_index=None, noise=None, noise_index=None, noise_offset=None, snr_db=None, out=None,
         max_len=None, max_rir_len=None, ws_bytes=None, rir_lengths=None, n_rir=None, out_stride=None):
    """-> (rc, out, gain).  `out` defaults to a NaN-filled [batch][out_stride]; every stride passed is the tensor's own."""
    lib = _native.lib()
    bsz = wave.shape[0]
    dt = _native.WAVE_I16 if wave.dtype == torch.int16 else _native.WAVE_F32
    if out is None:
        out = torch.full((bsz, out_stride), NAN, dtype=torch.float32, device="cuda")
    ptr = lambda t: None if t is None else t.data_ptr()
    rdata, rlen = rir if rir is not None else (None, None)
    rlen = rir_lengths if rir_lengths is not None else rlen
    ndata, nlen = noise if noise is not None else (None, None)
    mrl = max_rir_len if max_rir_len is not None else (int(rlen.max()) if rlen is not None else 0)
    need = lib.sir_reverb_workspace_bytes(fz.handle, bsz, max_len, min(mrl, 8192))
    assert need >= 4 * bsz
    ws = torch.zeros(need if ws_bytes is None else max(ws_bytes, 256), dtype=torch.uint8, device="cuda")
    snr = None if snr_db is None else torch.tensor(snr_db, dtype=torch.float32).cuda()
    keep = [i32(lengths), i32(rir_index), i32(noise_index), i32(noise_offset), snr]
    rc = lib.sir_wave_reverb_mix(fz.handle, wave.data_ptr(), dt, wave.stride(0), ptr(keep[0]),
                                 bsz, max_len, ptr(rdata), rdata.stride(0) if rdata is not None else 0, ptr(rlen),
                                 (rdata.shape[0] if rdata is not None else 0) if n_rir is None else n_rir, mrl, ptr(keep[1]),
                                 ptr(ndata), ndata.stride(0) if ndata is not None else 0, ptr(nlen),
                                 ndata.shape[0] if ndata is not None else 0, ptr(keep[2]), ptr(keep[3]), ptr(keep[4]),
                                 out.data_ptr(), out.stride(0), ws.data_ptr(),
                                 ws.numel() if ws_bytes is None else ws_bytes, _native.current_stream_ptr())
    torch.cuda.synchronize()
    return rc, out, ws[:4 * bsz].view(torch.float32).cpu().numpy().astype(np.float64)
