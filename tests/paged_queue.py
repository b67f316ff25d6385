"""The queue of the paged K/V cache tests, shared by tests/test_paged_host.py (the schedule on the host) and
tests/test_gpu_paged.py (the same schedule on the device): 14 requests, images on the even ones, budgets 1..24, four slots."""
N = 14
BUDGETS = [1, 2, 5, 9, 14, 20, 24, 3, 17, 8, 24, 12, 6, 21]
MAX_BATCH = 4
BLOCK = 16


def prompt_lens(Q: int):
    """positions of every prompt in the decoder: 32 + 3 r ids plus the Q image positions on the even requests, 20 + 3 r ids on the odd ones"""
    return [32 + 3 * r + Q if r % 2 == 0 else 20 + 3 * r for r in range(N)]


def has_image():
    return [r % 2 == 0 for r in range(N)]


def tight_pool_tokens(Q: int) -> int:
    """exactly the largest need of a single request: the smallest pool the queue is not refused with"""
    return max((t + b + BLOCK - 1) // BLOCK for t, b in zip(prompt_lens(Q), BUDGETS)) * BLOCK


def ample_pool_tokens(Q: int, ctx_max: int) -> int:
    """what the contiguous cache holds: nothing ever waits"""
    return MAX_BATCH * ctx_max
