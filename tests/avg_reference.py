"""References for DeviceAdamW's in-graph weight averaging (hri_emo_amd.optim, csrc/optim.hip): the float64 value of one averaging
update with the bound the fp32 kernel must meet, the fp32 weight the finalize kernel must produce bit for bit, and a host walk of
the device's bookkeeping (which event averages, n_averaged, w) that the tests compare with torch.optim.swa_utils.AveragedModel.

THE BOUND of ``avg_update_ref64``, every factor counted (u = 2^-24, the unit roundoff of fp32, round to nearest):
  the kernel computes, per element, d = fl(p - a) and then avg' = fl(w * d + a) as ONE fused multiply-add, from fp32 a, p and w.
    |d - (p - a)|            <= u |p - a|                          one rounding of the difference (exact in the normal range, a
                                                                  subnormal difference is exact as well)
    |avg' - (w d + a)|       <= u |w d + a| + 2^-150               one rounding of the fma (2^-150: half the smallest subnormal)
  with ref = a + w (p - a) in exact arithmetic:
    |w d + a - ref|          <= w u |p - a|                        the difference's rounding, scaled by w
    |w d + a|                <= |ref| + w u |p - a|
  so |avg' - ref| <= u (w |p - a| + |ref|) (1 + u) + 2^-150.
  The float64 evaluation of ref itself rounds three times (subtract, multiply, add), each <= 2^-53 relative of an intermediate no
  larger than |a| + w |p - a|: 3 * 2^-53 (|a| + w |p - a|) is added.  Nothing here is a measured number."""
import torch

U = 2.0 ** -24


def avg_update_ref64(a32, p32, w32):
    """a32, p32: fp32 tensors (the average in front of the update, the freshly updated parameters), w32: the fp32 weight the
    kernel used (0-dim tensor or float holding an fp32 value) -> (ref float64, bound float64), per element"""
    a, p, w = a32.double(), p32.double(), float(w32)
    diff = (p - a).abs()
    ref = a + w * (p - a)
    bound = U * (w * diff + ref.abs()) * (1.0 + U) + 2.0 ** -150 + 3 * 2.0 ** -53 * (a.abs() + w * diff)
    return ref, bound


def weight32(mode, n_before, decay):
    """the weight of an averaging update that finds n_before earlier ones, as the finalize kernel forms it: ONE fp32 operation on
    fp32 operands -- fl(1 - fl(decay)) for "ema", fl(1 / (n_before + 1)) for "swa" (n_before + 1 is exact in fp32) -> 0-dim fp32"""
    one = torch.ones((), dtype=torch.float32)
    if mode == "ema":
        return one - torch.tensor(decay, dtype=torch.float32)
    return one / torch.tensor(float(n_before + 1), dtype=torch.float32)


def walk(mode, decay, start, every, events):
    """the device's bookkeeping over a sequence of events "update" | "skip" | "hold" -> one record per event:
    (t, kind, n_averaged, w) with t the step count AFTER the event, kind in "none" | "first" | "update" | "untouched" (skip and
    hold: no word of avg_state is written), n_averaged after the event and w the fp32 weight written by it (None: not written)"""
    t, n, out = 0, 0, []
    for ev in events:
        if ev != "update":
            out.append((t, "untouched", n, None))
            continue
        t += 1
        if t > start and (t - start) % every == 0:
            out.append((t, "first" if n == 0 else "update", n + 1, weight32(mode, n, decay)))
            n += 1
        else:
            out.append((t, "none", n, None))
    return out
