"""What tests/test_idle_frames_host.py and tests/test_idle_frames_gpu.py share: the reference consumer's per-frame branch (lipreal.py:198-205, the same statements
as musereal.py:229-236) written out, with its own copy of the mirror walk (lipreal.py:65-72) so that nothing of the code under test is in the expectation."""


def mirror(size, index):
    turn = index // size
    res = index % size
    if turn % 2 == 0:
        return res
    return size - res - 1


class RefConsumer:
    """`process_frames` up to the choice of `combine_frame`, for one session: custom_lengths {audiotype: len(custom_img_cycle[audiotype])}, custom_index the
    consumer's OWN dict (it moves as the reference's does: one step per custom frame shown).  show() returns what the frame is made from instead of pixels."""

    def __init__(self, custom_lengths, custom_index):
        self.custom_lengths, self.custom_index = dict(custom_lengths), custom_index

    def show(self, idx, audio_frames):
        if audio_frames[0][1] != 0 and audio_frames[1][1] != 0:
            audiotype = audio_frames[0][1]
            if self.custom_index.get(audiotype) is not None:
                mirindex = mirror(self.custom_lengths[audiotype], self.custom_index[audiotype])
                self.custom_index[audiotype] += 1
                return ("custom", audiotype, mirindex)
            return ("idle", idx)
        return ("speech", idx)

    def batch(self, idxs, pairs):
        return [self.show(idxs[i], pairs[2 * i:2 * i + 2]) for i in range(len(idxs))]


def typed(types, chunk=None):
    """2B audio types -> 2B (pcm, type) pairs"""
    return [(chunk, int(t)) for t in types]
