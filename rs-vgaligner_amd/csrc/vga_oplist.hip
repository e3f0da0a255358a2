// vga_oplist.hip -- the table of the list makers and the part of their host frame that is no template (vga_oplist.hpp).
#include "vga_coverage.hpp"
#include "vga_deletion.hpp"
#include "vga_insertion.hpp"
#include "vga_pileup.hpp"

// in the order in which vga_align_batch counts the winners
const std::array<const oplist_maker *, 4> &oplist_makers()
{
    static const std::array<const oplist_maker *, 4> table = {&cov_maker(), &pu_maker(), &ia_maker(), &dl_maker()};
    return table;
}

// the counters of begin and reset are zeroed on the context's stream and waited for; the counts start again
static int oplist_zero(vga_ctx *ctx, const oplist_maker &m, oplist_state *s)
{
    for (const oplist_counter &c : m.counters(ctx->index, s))
        if (c.zeroed) VGA_HIP_CHECK(ctx, hipMemsetAsync(c.buf->p, 0, c.words * 4, ctx->stream));
    VGA_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
    s->n_alignments = 0;
    if (m.zero_own) m.zero_own(s);
    return VGA_OK;
}

int oplist_begin(vga_ctx *ctx, const oplist_maker &m, const char *fn)
{
    if (!ctx) return VGA_ERR_ARG;
    if (!ctx->index.loaded) return vga_set_error(ctx, VGA_ERR_NO_INDEX, OPLIST_ERR_NO_INDEX, fn);
    const vga_dev_index &ix = ctx->index;
    if (!m.fits(ix)) return vga_set_error(ctx, VGA_ERR_UNSUPPORTED, OPLIST_ERR_TOO_LARGE, fn, m.text.limit);
    (void)hipSetDevice(ctx->device);
    vga_ctx_scope scope(ctx);
    int rc = m.acquire(ctx, fn);
    if (rc != VGA_OK) return rc;
    oplist_state *s = m.counting(ctx);
    s->seq_length = (uint32_t)ix.seq_length;
    hipError_t e = hipSuccess;
    for (const oplist_counter &c : m.counters(ix, s))
        if (e == hipSuccess) e = c.buf->reserve(c.words);
    rc = e == hipSuccess ? oplist_zero(ctx, m, s) : vga_set_error(ctx, VGA_ERR_NOMEM, OPLIST_ERR_RESERVE, fn, hipGetErrorString(e));
    if (rc != VGA_OK) m.release(ctx);
    return rc;
}

int oplist_reset(vga_ctx *ctx, const oplist_maker &m, const char *fn)
{
    oplist_state *s = oplist_on(ctx, m, fn);
    if (!s) return VGA_ERR_ARG;
    (void)hipSetDevice(ctx->device);
    return oplist_zero(ctx, m, s);
}

int oplist_end(vga_ctx *ctx, const oplist_maker &m)
{
    if (!ctx) return VGA_ERR_ARG;
    (void)hipSetDevice(ctx->device);
    if (ctx->stream) (void)hipStreamSynchronize(ctx->stream);
    m.release(ctx);
    return VGA_OK;
}

oplist_state *oplist_on(vga_ctx *ctx, const oplist_maker &m, const char *fn)
{
    oplist_state *s = m.counting(ctx);
    if (!s) (void)vga_set_error(ctx, VGA_ERR_ARG, OPLIST_ERR_OFF, fn, m.text.name);
    return s;
}

int oplist_wrapped(vga_ctx *ctx, const oplist_state *s, const char *fn)
{
    if (s->n_alignments < 0xFFFFFFFFull) return VGA_OK;
    return vga_set_error(ctx, VGA_ERR_UNSUPPORTED, OPLIST_ERR_WRAPPED, fn, (unsigned long long)s->n_alignments);
}

