"""The host rules of ops.lora_add (DEVELOPMENT.md "Op argument contract"):
each is broken once, alone, on the smallest legal call, and must raise
before anything is launched, leaving y as it was. What lives in device memory
(the entries of perm and tiles) is the caller's obligation and gets no test
here: such a call cannot be rejected, only run."""
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda"
BF16, I32 = torch.bfloat16, torch.int32


@pytest.fixture(scope="module")
def ext():
    from llm_d_inference_scheduler_amd.ops import hip_ops
    return hip_ops()


def rnd(*shape, seed=0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g).to(BF16).to(DEV)


def legal():
    """T=1, in=32, out=16, S=1, R=16, one tile of one row."""
    return dict(y=rnd(1, 16), x=rnd(1, 32, seed=1), A=rnd(1, 16, 32, seed=2),
                B=rnd(1, 16, 16, seed=3),
                perm=torch.zeros(1, dtype=I32, device=DEV),
                tiles=torch.tensor([[0, 1, 0]], dtype=I32, device=DEV))


def strided(t):
    return torch.stack([t, t], dim=-1)[..., 0]


def misaligned(t):
    """t's values and shape at an address that is 2 bytes off 16."""
    flat = torch.empty(t.numel() + 8, dtype=t.dtype, device=t.device)
    out = flat[1:1 + t.numel()].view(t.shape)
    out.copy_(t)
    return out


BROKEN = [
    ("x", lambda a: a["x"].float(), "x must be"),
    ("x", lambda a: strided(a["x"]), "contiguous"),
    ("x", lambda a: a["x"].cpu(), "GPU"),
    ("x", lambda a: a["x"][0], "shape"),
    ("x", lambda a: misaligned(a["x"]), "aligned"),
    ("y", lambda a: a["y"].half(), "y must be"),
    ("y", lambda a: strided(a["y"]), "contiguous"),
    ("y", lambda a: rnd(2, 16), "shape"),
    ("y", lambda a: misaligned(a["y"]), "aligned"),
    (("x", "A"), lambda a: (rnd(1, 48), rnd(1, 16, 48)), "multiple of 32"),
    (("y", "B"), lambda a: (rnd(1, 24), rnd(1, 24, 16)), "multiple of 16"),
    ("A", lambda a: rnd(1, 16, 64), "shape"),
    ("A", lambda a: a["A"].float(), "A must be"),
    ("A", lambda a: a["A"].cpu(), "GPU"),
    ("A", lambda a: misaligned(a["A"]), "aligned"),
    (("A", "B"), lambda a: (rnd(0, 16, 32), rnd(0, 16, 16)), "slot"),
    (("A", "B"), lambda a: (rnd(1, 8, 32), rnd(1, 16, 8)), "rank"),
    (("A", "B"), lambda a: (rnd(1, 80, 32), rnd(1, 16, 80)), "rank"),
    ("B", lambda a: rnd(2, 16, 16), "shape"),
    ("B", lambda a: rnd(1, 32, 16), "shape"),
    ("B", lambda a: rnd(1, 16, 32), "shape"),
    ("B", lambda a: misaligned(a["B"]), "aligned"),
    ("perm", lambda a: a["perm"].long(), "perm must be"),
    ("perm", lambda a: torch.zeros(2, dtype=I32, device=DEV), "longer"),
    ("perm", lambda a: torch.zeros(1, 1, dtype=I32, device=DEV), "shape"),
    ("perm", lambda a: a["perm"].cpu(), "GPU"),
    ("tiles", lambda a: a["tiles"].long(), "tiles must be"),
    ("tiles", lambda a: torch.zeros(1, 2, dtype=I32, device=DEV), "shape"),
    ("tiles", lambda a: torch.zeros(3, dtype=I32, device=DEV), "shape"),
    ("tiles", lambda a: a["tiles"].cpu(), "GPU"),
]


def test_smallest_legal_call_runs_and_matches_ref(ext):
    from llm_d_inference_scheduler_amd.ops import ref
    a = legal()
    want = a["y"].cpu()
    ref.lora_add(want, a["x"].cpu(), a["A"].cpu(), a["B"].cpu(),
                 a["perm"].cpu(), a["tiles"].cpu())
    ext.lora_add(*a.values())
    torch.testing.assert_close(a["y"].cpu().float(), want.float(),
                               rtol=2 ** -7, atol=2 ** -7)


@pytest.mark.parametrize("i", range(len(BROKEN)),
                         ids=[f"{i}-{b[0]}" for i, b in enumerate(BROKEN)])
def test_broken_rule_raises_and_leaves_y(ext, i):
    names, make, message = BROKEN[i]
    a = legal()
    new = make(a)
    if isinstance(names, str):
        names, new = (names,), (new,)
    a.update(dict(zip(names, new)))
    y = a["y"]
    before = y.clone()
    with pytest.raises(RuntimeError, match=message):
        ext.lora_add(*a.values())
    torch.cuda.synchronize()
    assert torch.equal(y.cpu().float(), before.cpu().float())
