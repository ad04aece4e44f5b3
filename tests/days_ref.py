"""Python restatement of the reference's day sampler (include/utilities/sampler.h:29-46): one
std::default_random_engine (libstdc++: minstd_rand0, x <- 16807 x mod 2^31 - 1) per sampler, seeded with an
unsigned, and std::uniform_int_distribution<size_t>{0, n - 1} in libstdc++'s downscaling form.  test_days_abi.py
pins it against libstdc++ itself; the GPU tests hold days_draw_kernel to it."""

M31 = 2147483647


def seed_state(seed):
    """std::minstd_rand0(seed) with seed an unsigned: x = seed mod (2^31 - 1), 0 -> 1."""
    x = (seed & 0xFFFFFFFF) % M31
    return 1 if x == 0 else x


def draw(x, n):
    """One uniform_int_distribution<size_t>{0, n - 1}(rng) from state x: (new state, value)."""
    scaling = 2147483645 // n
    past = n * scaling
    while True:
        x = x * 16807 % M31
        if x - 1 < past:
            return x, (x - 1) // scaling


def book_days(seed, gid, n, draws):
    """The first `draws` days (0 .. n - 1) global book `gid` draws with the engine's seed."""
    x = seed_state(seed + gid)
    out = []
    for _ in range(draws):
        x, v = draw(x, n)
        out.append(v)
    return out
