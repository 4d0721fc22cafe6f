// IngestReq, what a txo_ingest_u8* entry asks for, and IngestPlan, the request behind every refusal that needs neither an engine nor a
// device, as values; the pieces of the rule that txo_ingest_box / _fit / _fit_scratch / _trim_views share with them.  Host code, included
// by engine.hip only (after every kernel header: it reads ingest.h's and ingest_fit.h's constants).
#pragma once

namespace txo {

// The list of source images as the caller gave it: image b is shapes[3 b ..] = (h, w, ch) bytes, rows tightly packed, offsets[b] bytes behind pix
struct IngestList { const unsigned char* pix = nullptr; const int64_t* offsets = nullptr; const int32_t* shapes = nullptr; int B = 0; };

// One container ingest, what txo_ingest_u8 / _fit / _view ask for (texocr.h says what each argument is).
struct IngestReq {
    txo_engine* engine = nullptr;         // the handle as given: a null one is refused with the other null arguments, behind every other check
    IngestList src;
    bool view = false;                    // a rectangle of every image takes its place (txo_ingest_u8_view) ...
    const int32_t* views = nullptr;       // ... [B][4] = (y0, x0, h', w') in source pixels (a null array is then refused, behind the list)
    bool fit = false; int Fh = 0, Fw = 0; // images beyond Fh x Fw are downscaled first (txo_ingest_u8_fit; _view unless Fh = Fw = 0); the target is judged then
    int C = 0, Hc = 0, Wc = 0;            // the container [B][C][Hc][Wc] ...
    float* box = nullptr; int32_t* sizes_out = nullptr;   // ... on the device, and where the sizes of its images go on the host [B][2]
    void* scratch = nullptr; long long scratch_bytes = 0; // the intermediates of the fit's horizontal passes (device)
};

// The request behind ingest_plan's checks, what Engine::ingest takes.  The three arrays are the caller's own for whole images and the
// plan's vectors for views, which fold their origins into the offsets; nothing is copied twice.
struct IngestPlan {
    const int64_t* off = nullptr;         // [B] first byte of what the kernels read of image b
    const int32_t* shapes = nullptr;      // [B][3] its (h, w, ch)
    const int32_t* pitch = nullptr;       // [B] pixels from one of its rows to the next; null: every row follows the last (no view is narrower than its image)
    std::vector<int32_t> fitted;          // [B][2] (h', w') under the fit target; empty: no fit was asked for
    bool oversized = false;               // some image is downscaled; otherwise the call is plain ingest's own launch, bit for bit
    long long scratch_need = 0;           // bytes of the horizontal passes' intermediates
    std::vector<int64_t> voff; std::vector<int32_t> vshapes, vpitch;   // what off / shapes / pitch point at for a list of views
    int out_h(int b) const { return fitted.empty() ? shapes[3 * b] : fitted[2 * b]; }           // the size image b has in the container
    int out_w(int b) const { return fitted.empty() ? shapes[3 * b + 1] : fitted[2 * b + 1]; }
};

static inline long long ingest_round16(long long v) { return (v + 15) / 16 * 16; }

// shapes int32 [B][3] = (h, w, ch); every message names the image.  box (may be null): the largest rounded-up height / width
static int ingest_check_shapes(const int32_t* shapes, int B, long long* box) {
    if (B < 1) return fail(TXO_E_INVALID, "ingest: no images (B must be >= 1)");
    if (!shapes) return fail(TXO_E_INVALID, "ingest: null shapes");
    if (B > 65535) return fail(TXO_E_INVALID, "ingest: more than 65535 images in one call");
    long long H = 0, W = 0;
    for (int b = 0; b < B; ++b) {
        const int h = shapes[3 * b], w = shapes[3 * b + 1], ch = shapes[3 * b + 2];
        const std::string who = "ingest: image " + std::to_string(b);
        if (ch != 1 && ch != 3 && ch != 4)
            return fail(TXO_E_INVALID, who + " has ch = " + std::to_string(ch) + "; the channel count must be 1 (L), 3 (RGB) or 4 (RGBA)");
        if (h < 1 || w < 1) return fail(TXO_E_INVALID, who + " is " + std::to_string(h) + "x" + std::to_string(w) + "; both sides must be >= 1");
        H = std::max(H, ingest_round16(h)); W = std::max(W, ingest_round16(w));
    }
    if (box) { box[0] = H; box[1] = W; }
    return 0;
}

static int ingest_check_offset(long long off, int b) {
    return off < 0 ? fail(TXO_E_INVALID, "ingest: image " + std::to_string(b) + " has a negative byte offset") : 0;
}

// The fit rule over a list that has passed ingest_check_shapes: fitted (may be null) [B][2] = (h', w') of every image under the target
// (Fh, Fw), scratch (may be null) the bytes of the horizontal passes' intermediates.  Refuses a bad target and an axis that shrinks too far.
static_assert(TXO_FIT_TAPS == FIT_TAPS, "texocr.h and ingest_fit.h disagree on the taps per output pixel");
struct FitTarget { int Fh, Fw; };
static int ingest_fit_sizes(const int32_t* shapes, int B, FitTarget t, int32_t* fitted, long long* scratch) {
    const int Fh = t.Fh, Fw = t.Fw;
    if (Fh < 16 || Fh % 16 || Fw < 16 || Fw % 16)
        return fail(TXO_E_INVALID, "ingest: the fit target is " + std::to_string(Fh) + "x" + std::to_string(Fw) + "; both sides must be positive multiples of 16");
    if ((32LL * Fh + FR_ROWS - 1) / FR_ROWS > 65535) return fail(TXO_E_INVALID, "ingest: the fit target's height exceeds the launch grid");
    long long need = 0;
    for (int b = 0; b < B; ++b) {
        const int h = shapes[3 * b], w = shapes[3 * b + 1];
        int fh, fw;
        fit_size(h, w, Fh, Fw, &fh, &fw);
        if ((long long)h > (long long)FIT_MAX_SCALE * fh || (long long)w > (long long)FIT_MAX_SCALE * fw)
            return fail(TXO_E_INVALID, "ingest: image " + std::to_string(b) + " is " + std::to_string(h) + "x" + std::to_string(w) + ", " + std::to_string(fh) + "x" +
                                           std::to_string(fw) + " fitted to " + std::to_string(Fh) + "x" + std::to_string(Fw) + ": an axis shrinks by more than " +
                                           std::to_string(FIT_MAX_SCALE) + " times");
        if (fitted) { fitted[2 * b] = fh; fitted[2 * b + 1] = fw; }
        if (fw != w) need += ingest_fit_mid_bytes(h, fw, shapes[3 * b + 2]);
    }
    if (scratch) *scratch = need;
    return 0;
}

// The trim rule of texocr.h "Trim-to-ink ingest": ink extents (ymin, xmin, ymax, xmax; ymax < 0: no ink) of an image (h, w) and a margin ->
// the view (y0, x0, h', w'): the ink box widened by the margin on every side and clamped to the image; the whole image where there is no ink
static inline void trim_view_of(const int* ext, int h, int w, int margin, int32_t* view) {
    if (ext[2] < 0) { view[0] = 0; view[1] = 0; view[2] = h; view[3] = w; return; }
    const long long y0 = std::max(0LL, (long long)ext[0] - margin), y1 = std::min((long long)h, (long long)ext[2] + 1 + margin);
    const long long x0 = std::max(0LL, (long long)ext[1] - margin), x1 = std::min((long long)w, (long long)ext[3] + 1 + margin);
    view[0] = (int32_t)y0; view[1] = (int32_t)x0; view[2] = (int32_t)(y1 - y0); view[3] = (int32_t)(x1 - x0);
}

// Every refusal of a container ingest that needs neither an engine nor a device, in the order the C entry points report: the list; the
// views; the fit target and the scale limit; the container, judged on the sizes that will be written; the scratch; the null arguments;
// the container's alignment.  On 0 *p is the request as Engine::ingest takes it.
static int ingest_plan(const IngestReq& q, IngestPlan* p) {
    const IngestList& l = q.src;
    const int B = l.B;
    if (int r = ingest_check_shapes(l.shapes, B, nullptr)) return r;
    p->off = l.offsets; p->shapes = l.shapes;
    if (q.view) {
        if (!l.offsets) return fail(TXO_E_INVALID, "ingest: null offsets");
        if (!q.views) return fail(TXO_E_INVALID, "ingest: null views");
        p->voff.resize((size_t)B); p->vshapes.resize((size_t)3 * B); p->vpitch.resize((size_t)B);
        bool whole = true;                                            // every view spans its image's rows: nothing is pitched
        for (int b = 0; b < B; ++b) {
            const long long h = l.shapes[3 * b], w = l.shapes[3 * b + 1], ch = l.shapes[3 * b + 2];
            const long long y0 = q.views[4 * b], x0 = q.views[4 * b + 1], vh = q.views[4 * b + 2], vw = q.views[4 * b + 3];
            const std::string who = "ingest: image " + std::to_string(b) + " has the view " + std::to_string(vh) + "x" + std::to_string(vw) + " at (" +
                                    std::to_string(y0) + ", " + std::to_string(x0) + ")";
            if (int r = ingest_check_offset(l.offsets[b], b)) return r;
            if (vh < 1 || vw < 1) return fail(TXO_E_INVALID, who + "; both sides must be >= 1");
            if (y0 < 0 || x0 < 0 || y0 + vh > h || x0 + vw > w)
                return fail(TXO_E_INVALID, who + ", which reaches outside the image's " + std::to_string(h) + "x" + std::to_string(w));
            p->vshapes[3 * b] = (int32_t)vh; p->vshapes[3 * b + 1] = (int32_t)vw; p->vshapes[3 * b + 2] = (int32_t)ch;
            p->voff[b] = l.offsets[b] + (y0 * w + x0) * ch;           // the origin folds into the offset; the rows stay w pixels apart
            p->vpitch[b] = (int32_t)w;
            whole = whole && vw == w;
        }
        p->off = p->voff.data(); p->shapes = p->vshapes.data();
        p->pitch = whole ? nullptr : p->vpitch.data();                // (views that keep their images' widths are tightly packed images)
    }
    if (q.fit) {
        p->fitted.resize((size_t)2 * B);
        if (int r = ingest_fit_sizes(p->shapes, B, {q.Fh, q.Fw}, p->fitted.data(), &p->scratch_need)) return r;
        for (int b = 0; b < B; ++b) p->oversized = p->oversized || p->fitted[2 * b] != p->shapes[3 * b] || p->fitted[2 * b + 1] != p->shapes[3 * b + 1];
    }
    if (!p->off) return fail(TXO_E_INVALID, "ingest: null offsets");
    if (q.C < 1) return fail(TXO_E_INVALID, "ingest: the container's channel count must be >= 1");
    if (q.Hc < 1 || q.Wc < 1) return fail(TXO_E_INVALID, "ingest: the container's height/width must be positive");
    if (q.Wc % 4) return fail(TXO_E_INVALID, "ingest: the container's width must be a multiple of 4 (rows are written in 16-byte pieces)");
    if ((q.Hc + IG_ROWS - 1) / IG_ROWS > 65535) return fail(TXO_E_INVALID, "ingest: the container's height exceeds the launch grid");
    for (int b = 0; b < B; ++b) {
        const long long h16 = ingest_round16(p->out_h(b)), w16 = ingest_round16(p->out_w(b));
        if (int r = ingest_check_offset(p->off[b], b)) return r;
        if (h16 > q.Hc || w16 > q.Wc)
            return fail(TXO_E_INVALID, "ingest: image " + std::to_string(b) + " is " + std::to_string(p->out_h(b)) + "x" + std::to_string(p->out_w(b)) + ", " +
                                           std::to_string(h16) + "x" + std::to_string(w16) + " rounded up to multiples of 16: it does not fit the container's " +
                                           std::to_string(q.Hc) + "x" + std::to_string(q.Wc));
    }
    if (p->scratch_need > 0 && (!q.scratch || q.scratch_bytes < p->scratch_need))
        return fail(TXO_E_INVALID, "ingest: the fit scratch is " + (q.scratch ? std::to_string(q.scratch_bytes) + " bytes" : std::string("null")) +
                                       "; the horizontal passes of this list need " + std::to_string(p->scratch_need) + " bytes (txo_ingest_fit_scratch)");
    if (!q.engine || !l.pix || !q.box || !q.sizes_out) return fail(TXO_E_INVALID, "ingest: null argument");
    if (reinterpret_cast<uintptr_t>(q.box) % 16) return fail(TXO_E_INVALID, "ingest: the container must be 16-byte aligned (rows are written in 16-byte pieces)");
    return 0;
}

}  // namespace txo
