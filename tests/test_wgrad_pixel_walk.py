"""CPU tier: the mixed-radix pixel walk of wgrad_x6_kernel (csrc/wgrad_x6.hip, `fetch`) restated in
Python and compared with divmod.  A thread holds (image, row, column) of its output pixel and
advances 32 pixels per chunk by (step_img, step_ho, step_wo) with one conditional carry per digit;
the walk must name pixel c*32 + j of every chunk c, for maps larger and smaller than a chunk."""
import pytest


def walk(Ho, Wo, first, chunks):
    """the q_* / step_* recurrence, exactly as the kernel writes it"""
    HoWo = Ho * Wo
    q_img = first // HoWo
    rem = first - q_img * HoWo
    q_ho = rem // Wo
    q_wo = rem - q_ho * Wo
    step_img = 32 // HoWo
    step_ho = (32 - step_img * HoWo) // Wo
    step_wo = 32 - step_img * HoWo - step_ho * Wo
    for _ in range(chunks):
        yield q_img, q_ho, q_wo
        q_wo += step_wo
        if q_wo >= Wo:
            q_wo -= Wo
            q_ho += 1
        q_ho += step_ho
        if q_ho >= Ho:
            q_ho -= Ho
            q_img += 1
        q_img += step_img


@pytest.mark.parametrize("Ho,Wo", [(1, 1), (2, 2), (3, 3), (4, 4), (1, 5), (5, 1), (2, 16), (16, 2), (4, 8),
                                   (8, 4), (1, 32), (32, 1), (3, 11), (8, 9), (9, 10), (7, 6), (5, 7),
                                   (1, 33), (33, 1), (16, 16), (64, 64), (31, 1), (1, 31), (6, 5)])
def test_pixel_walk_matches_divmod(Ho, Wo):
    HoWo = Ho * Wo
    for first_chunk in (0, 1, 7):                   # c_first of a slice of the pixels
        for j in range(32):                         # pp * 2 + e: the thread's pixel of a chunk
            first = first_chunk * 32 + j
            for c, got in enumerate(walk(Ho, Wo, first, 40)):
                m = first + c * 32
                img, rem = divmod(m, HoWo)
                assert got == (img,) + divmod(rem, Wo), (Ho, Wo, first, c)
