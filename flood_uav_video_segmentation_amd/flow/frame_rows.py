"""FrameRows: the chunked per-frame device tables behind every report of flow/predict.py and flow/mosaic.py."""
import torch


class FrameRows:
    """One stage's per-frame device tables: parallel buffers, `spec` = one (shape of a frame's rows, dtype) each, allocated a chunk of
    frames at a time -- one allocation per chunk, not one per window -- and filled in frame order; nothing is read back before a report
    asks.  Every chunk is zero-filled: the reports trim a frame's rows by a counts column and hand out rows nobody wrote.  The chunk
    size is an argument of every call, not kept here: the predictor's REPORT_CHUNK, outline_chunk and simple_chunk may be set at any
    time before the first window, and without a reference back to the predictor the buffers are freed with it."""

    def __init__(self, *spec):
        self.spec = spec
        self.clear()

    def clear(self):
        self.chunks = []  # one tuple of buffers [chunk, *shape] per chunk, in frame order
        self.frames = 0   # frames written: the newest chunk is filled up to frames % chunk

    def rows(self, row, take, chunk, device):
        """Views of rows row .. row + take - 1 of the newest chunk, one per buffer; row == 0 starts a new chunk on `device`.  Called
        directly by a table that keeps in step with another one's pieces(): that one counts the frames for both."""
        if row == 0:
            self.chunks.append(tuple(torch.zeros((chunk,) + tuple(shape), dtype=dtype, device=device) for shape, dtype in self.spec))
        return tuple(b[row:row + take] for b in self.chunks[-1])

    def pieces(self, n, chunk, device):
        """The next n frames, cut at the chunk borders: yields (done, take, row, views) -- frames done .. done + take - 1 of the n go
        into rows row .. of the newest chunk, which `views` are.  The frames count once the caller comes back for the next piece."""
        done = 0
        while done < n:
            row = self.frames % chunk
            take = min(n - done, chunk - row)
            yield done, take, row, self.rows(row, take, chunk, device)
            done += take
            self.frames += take

    def filled(self, chunk, *followers):
        """Chunk by chunk (take, views of the rows written), for a report that reads back one chunk at a time; with followers -- tables
        kept in step with this one through rows() -- the views of each of them after its own."""
        left = self.frames
        for i, buffers in enumerate(self.chunks):
            take = min(left, chunk)
            yield (take,) + tuple(tuple(b[:take] for b in t.chunks[i]) for t in (self,) + followers)
            left -= take

    def flat(self):
        """The first buffer's rows written, as ONE device tensor (a copy), for a report that reads back once."""
        return torch.cat([buffers[0] for buffers in self.chunks])[:self.frames]
