"""Independent scalar reference of csrc/kernels/common.h::feistel_perm in Python integers, shared by the CPU
permutation suite and the GPU suites."""

_MASK64 = (1 << 64) - 1


def py_mix(z: int) -> int:
    z &= _MASK64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & _MASK64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & _MASK64
    return z ^ (z >> 31)


def py_perm(i: int, n: int, seed: int, epoch: int) -> int:
    """perm(i) of FeistelPermutation(n, seed, epoch): six rounds, cycle walking while outside [0, n)."""
    from ddl_amd.permutation import half_bits_for, round_keys

    keys = round_keys(seed, epoch)
    h = half_bits_for(n)
    mask = (1 << h) - 1

    def once(x):
        left, right = x >> h, x & mask
        for k in keys:
            left, right = right, left ^ (py_mix(right ^ k) & mask)
        return (left << h) | right

    x = once(i)
    while x >= n:
        x = once(x)
    return x


def py_position(row: int, n: int, seed: int, epoch: int) -> int:
    """The position p with py_perm(p) == row: the rounds backwards, walking while outside [0, n)."""
    from ddl_amd.permutation import half_bits_for, round_keys

    keys = round_keys(seed, epoch)
    h = half_bits_for(n)
    mask = (1 << h) - 1

    def back(x):
        left, right = x >> h, x & mask
        for k in reversed(keys):
            left, right = right ^ (py_mix(left ^ k) & mask), left
        return (left << h) | right

    x = back(row)
    while x >= n:
        x = back(x)
    assert py_perm(x, n, seed, epoch) == row
    return x
