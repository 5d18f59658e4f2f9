"""GPU tier of the prefix-cache tests: the cases of tests/prefix_cases.py run
through the `_hip_ops` extension on the device and are compared bitwise (or
as sorted (key, mask) lists, where placement depends on thread order) with
the model in ops.ref. tests/test_prefix_cases.py shows on the CPU that these
cases can fail. The whole file takes a few seconds."""
import numpy as np
import pytest
import torch

import prefix_cases as pc

pytestmark = pytest.mark.gpu

DEV = "cuda"


@pytest.fixture(scope="module")
def ext():
    from llm_d_inference_scheduler_amd.ops import hip_ops
    return hip_ops()


@pytest.mark.parametrize("case", pc.KERNEL_CASES, ids=lambda c: c.__name__)
def test_kernel_case(ext, case):
    case(ext, DEV)


def test_history_matches_host_index_on_device():
    idx = pc.check_history(DEV, seed=0)
    assert idx.keys.is_cuda


def test_mixed_model_batch_on_device():
    pc.check_mixed_models(DEV)


class TestBindingChecks:
    """Bad arguments are rejected on the host, before any launch: the call
    raises and the table is untouched."""

    @pytest.fixture()
    def t(self):
        class T:
            keys = torch.zeros(16, dtype=torch.uint64, device=DEV)
            masks = torch.zeros(16, dtype=torch.uint64, device=DEV)
            hashes = pc.u64(np.arange(2, 10).reshape(2, 4), DEV)
            counts = torch.full((2,), 4, dtype=torch.int32, device=DEV)
            dropped = torch.zeros(1, dtype=torch.int32, device=DEV)
            tokens = torch.arange(8, dtype=torch.int32, device=DEV)
            offsets = torch.tensor([0, 8], dtype=torch.int64, device=DEV)
        yield T
        assert not T.keys.view(torch.int64).any()
        assert not T.masks.view(torch.int64).any()
        assert int(T.dropped.item()) == 0

    @pytest.mark.parametrize("endpoint", [-1, 64, 1 << 40])
    def test_table_update_endpoint(self, ext, t, endpoint):
        for remove in (False, True):
            with pytest.raises(RuntimeError, match="endpoint"):
                ext.table_update(t.keys, t.masks, t.hashes, endpoint, remove,
                                 t.dropped)

    @pytest.mark.parametrize("n_endpoints", [0, -1, 65])
    def test_match_n_endpoints(self, ext, t, n_endpoints):
        with pytest.raises(RuntimeError, match="n_endpoints"):
            ext.match_longest(t.keys, t.masks, t.hashes, t.counts,
                              n_endpoints)

    @pytest.mark.parametrize("block_tokens,max_blocks",
                             [(0, 4), (-1, 4), (4, 0), (4, -3)])
    def test_hash_sizes(self, ext, t, block_tokens, max_blocks):
        with pytest.raises(RuntimeError, match="must be >= 1"):
            ext.hash_prompts(t.tokens, t.offsets, block_tokens, max_blocks, 1)

    def test_hash_offsets_empty(self, ext, t):
        with pytest.raises(RuntimeError, match="offsets"):
            ext.hash_prompts(t.tokens, t.offsets[:0], 4, 4, 1)

    @pytest.mark.parametrize("which", ["keys", "masks", "hashes"])
    def test_uint64_only(self, ext, t, which):
        args = {"keys": t.keys, "masks": t.masks, "hashes": t.hashes}
        args[which] = args[which].view(torch.int64)
        with pytest.raises(RuntimeError, match="uint64"):
            ext.table_update(args["keys"], args["masks"], args["hashes"], 0,
                             False, t.dropped)
        with pytest.raises(RuntimeError, match="uint64"):
            ext.match_longest(args["keys"], args["masks"], args["hashes"],
                              t.counts, 4)

    @pytest.mark.parametrize("which", ["keys", "masks", "hashes"])
    def test_one_device(self, ext, t, which):
        args = {"keys": t.keys, "masks": t.masks, "hashes": t.hashes}
        args[which] = args[which].cpu()
        with pytest.raises(RuntimeError):
            ext.table_update(args["keys"], args["masks"], args["hashes"], 0,
                             False, t.dropped)
        with pytest.raises(RuntimeError):
            ext.match_longest(args["keys"], args["masks"], args["hashes"],
                              t.counts, 4)

    def test_keys_and_masks_equally_long(self, ext, t):
        with pytest.raises(RuntimeError, match="equally long"):
            ext.table_update(t.keys, t.masks[:8], t.hashes, 0, False,
                             t.dropped)
        with pytest.raises(RuntimeError, match="equally long"):
            ext.match_longest(t.keys[:8], t.masks, t.hashes, t.counts, 4)

    def test_table_cap_power_of_two(self, ext, t):
        with pytest.raises(RuntimeError, match="2\\^k"):
            ext.table_update(t.keys[:12], t.masks[:12], t.hashes, 0, False,
                             t.dropped)

    def test_match_hashes_2d(self, ext, t):
        with pytest.raises(RuntimeError, match="max_blocks"):
            ext.match_longest(t.keys, t.masks, t.hashes.view(-1), t.counts, 4)

    def test_match_counts_per_row(self, ext, t):
        with pytest.raises(RuntimeError, match="counts"):
            ext.match_longest(t.keys, t.masks, t.hashes, t.counts[:1], 4)
        with pytest.raises(RuntimeError, match="counts"):
            ext.match_longest(t.keys, t.masks, t.hashes,
                              t.counts.to(torch.int64), 4)

    def test_dropped_counter_type(self, ext, t):
        with pytest.raises(RuntimeError, match="dropped"):
            ext.table_update(t.keys, t.masks, t.hashes, 0, False,
                             t.dropped.to(torch.int64))
        with pytest.raises(RuntimeError, match="dropped"):
            ext.table_update(t.keys, t.masks, t.hashes, 0, False,
                             torch.zeros(2, dtype=torch.int32, device=DEV))

    def test_good_arguments_still_work(self, ext):
        keys = torch.zeros(16, dtype=torch.uint64, device=DEV)
        masks = torch.zeros(16, dtype=torch.uint64, device=DEV)
        h = pc.u64([[5, 6, 7]], DEV)
        ext.table_update(keys, masks, h, 63, False)     # counter is optional
        c = torch.tensor([3], dtype=torch.int32, device=DEV)
        out = ext.match_longest(keys, masks, h, c, 64).cpu()
        assert out[0, 63] == 3 and int(out.sum()) == 3
