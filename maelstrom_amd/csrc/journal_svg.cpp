// journal_svg.cpp — msim_journal_svg_rows: one journal as the Lamport diagram the reference draws from it (net/viz.clj:60-108,145-259,
// 281-325): a column per endpoint, a row per event, an arrow per delivered message.  The contract is include/maelsim_journal.h's
// last section; the geometry is computed in doubles and printed to four decimals.  Host only, no device.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <string>
#include <unordered_map>
#include <vector>

#include "../../include/maelsim.h"
#include "journal_names.h"

namespace {

constexpr uint32_t LIMIT = 10000;   // events drawn (viz.clj:13-16)
constexpr double WIDTH = 1200.0, Y_STEP = 20.0;

void num(std::string &o, double v) {
  char b[40];
  std::snprintf(b, sizeof b, "%.4f", v);
  o += b;
}

struct Column { uint32_t rank; std::string name; uint32_t endpoint; };   // rank 0: c<k> / n<k> by (letter, k); 1: a service, by name

}  // namespace

extern "C" int msim_journal_svg_rows(const msim_config *cfg, const msim_event *events, uint32_t n_events, char *out, size_t cap, size_t *needed) {
  if (!cfg || (!events && n_events) || (!out && cap)) return MSIM_E_INVALID;
  const uint32_t N = cfg->n_nodes, slots = std::max(cfg->concurrency, N);
  // the window: no init traffic, the events up to position 10000 + 4 n + 1, of those the first 10000
  std::vector<uint32_t> win;
  const uint64_t bound = (uint64_t)LIMIT + 4ull * N + 1ull;
  for (uint32_t i = 0; i < n_events && i < bound; i++) {
    const uint32_t type = events[i].msg & 0x7Fu;
    if (type == 0 || type >= sizeof journal_names::MSG_TYPES / sizeof journal_names::MSG_TYPES[0]) return MSIM_E_RANGE;
    if (type != MSIM_M_INIT && type != MSIM_M_INIT_OK) win.push_back(i);
  }
  const bool truncated = win.size() > LIMIT;
  if (truncated) win.resize(LIMIT);
  const uint32_t steps = (uint32_t)win.size();
  // the columns: the endpoints that occur, clients, then nodes, then the services by name
  bool seen[256] = {false};
  for (uint32_t i : win) { seen[events[i].route & 0xFFu] = true; seen[(events[i].route >> 8) & 0xFFu] = true; }
  std::vector<Column> cols;
  for (uint32_t e = 0; e < 256; e++)
    if (seen[e]) cols.push_back(Column{e >= N + slots ? 1u : 0u, journal_names::endpoint(e, N, slots, cfg), e});
  std::sort(cols.begin(), cols.end(), [&](const Column &a, const Column &b) {
    if (a.rank != b.rank) return a.rank < b.rank;
    if (a.rank) return a.name != b.name ? a.name < b.name : a.endpoint < b.endpoint;
    const bool ac = a.endpoint >= N, bc = b.endpoint >= N;   // "c" sorts in front of "n"
    return ac != bc ? ac : a.endpoint < b.endpoint;
  });
  double col_x[256] = {0};
  for (size_t k = 0; k < cols.size(); k++) col_x[cols[k].endpoint] = ((double)k + 0.5) / (double)cols.size() * WIDTH;
  const auto y = [](double step) { return Y_STEP * (1.5 + step); };
  const auto client = [&](uint32_t e) { return e - N < slots; };

  std::string o;
  o.reserve((size_t)steps * 400 + 4096);
  o += "<?xml version=\"1.0\" encoding=\"UTF-8\"?>\n<svg xmlns=\"http://www.w3.org/2000/svg\" xmlns:xlink=\"http://www.w3.org/1999/xlink\" version=\"2.0\" width=\"1200\" height=\"";
  num(o, Y_STEP * (7.0 + steps));
  o += "\">\n<style>svg { font-family: Helvetica, Arial, sans-serif; font-size: 11px; } rect { stroke: #fff; stroke-width: 3; stroke-linecap: butt; } polygon { fill: #000; }</style>\n"
       "<defs><polygon id=\"ahead\" points=\"0 0, -12 4, -12 -4\"/>"
       "<filter id=\"glow\" x=\"0\" y=\"0\"><feGaussianBlur in=\"SourceAlpha\" stdDeviation=\"2\" result=\"blurred\"/><feFlood flood-color=\"#fff\"/>"
       "<feComposite operator=\"in\" in2=\"blurred\"/><feComponentTransfer><feFuncA type=\"linear\" slope=\"10\" intercept=\"0\"/></feComponentTransfer>"
       "<feMerge><feMergeNode/><feMergeNode in=\"SourceGraphic\"/></feMerge></filter></defs>\n";
  // the endpoints' names every 50 steps, a line per endpoint
  o += "<g class=\"node-labels\">\n";
  for (const Column &c : cols)
    for (uint32_t step = 0; step < steps; step += 50) {
      o += "<text x=\""; num(o, col_x[c.endpoint]); o += "\" y=\""; num(o, y((double)step - 0.5));
      o += "\" text-anchor=\"middle\" alignment-baseline=\"middle\" fill=\""; o += step ? "#aaa" : "#000"; o += "\">" + c.name + "</text>\n";
    }
  o += "</g>\n<g class=\"node-lines\">\n";
  for (const Column &c : cols) {
    o += "<line stroke=\"#ccc\" x1=\""; num(o, col_x[c.endpoint]); o += "\" y1=\""; num(o, y(0)); o += "\" x2=\""; num(o, col_x[c.endpoint]);
    o += "\" y2=\""; num(o, y((double)steps + 1.0)); o += "\"/>\n";
  }
  // an arrow per :recv whose :send lies in the window: from (the send's src, its step) to (the recv's dest, its step)
  o += "</g>\n<g class=\"messages\">\n";
  struct From { uint32_t endpoint, step; };
  std::unordered_map<uint32_t, From> froms;
  for (uint32_t k = 0; k < steps; k++) {
    const msim_event &e = events[win[k]];
    const uint32_t id = e.msg >> 8, src = e.route & 0xFFu, dest = (e.route >> 8) & 0xFFu, type = e.msg & 0x7Fu, step = k + 1;
    if (!(e.msg & 0x80u)) { froms[id] = From{src, step}; continue; }
    const auto f = froms.find(id);
    if (f == froms.end()) continue;   // (the reference asserts; a recv without its send is not drawn)
    const double x0 = col_x[f->second.endpoint], y0 = y(f->second.step), x1 = col_x[dest], y1 = y(step);
    const double length = std::sqrt((x1 - x0) * (x1 - x0) + (y1 - y0) * (y1 - y0)), angle = std::atan2(y1 - y0, x1 - x0) / 2.0 / M_PI * 360.0;
    const bool left = !(-90.0 < angle && angle < 90.0);
    const char *fill = type == MSIM_M_ERROR ? "#FF1E90" : (client(src) || client(dest)) ? "#81BFFC" : "#000";
    const std::string what = journal_names::MSG_TYPES[type];
    o += "<g transform=\"translate("; num(o, x0); o += " "; num(o, y0); o += ") rotate("; num(o, angle); o += ")\">";
    o += "<rect x=\"0\" y=\"-2.5\" height=\"5\" width=\""; num(o, length - 4.0); o += "\" fill=\""; o += fill; o += "\"><title>";
    o += journal_names::endpoint(src, N, slots, cfg) + " \xE2\x86\x92 " + journal_names::endpoint(dest, N, slots, cfg) + " " + what + "</title></rect>";
    o += "<use xlink:href=\"#ahead\" x=\""; num(o, length); o += "\" y=\"0\"/>";
    for (int glow = 1; glow >= 0; glow--) {   // the label's glow, then the label
      o += "<text text-anchor=\"middle\" x=\""; num(o, length / 2.0); o += "\" y=\""; num(o, -Y_STEP / 5.0); o += "\"";
      if (left) { o += " transform=\"rotate(180 "; num(o, length / 2.0); o += " 0)\""; }
      if (glow) o += " filter=\"url(#glow)\" style=\"fill: #fff\"";
      o += ">" + what + "</text>";
    }
    o += "</g>\n";
  }
  o += "</g>\n";
  if (truncated) {
    const double step = (double)steps + 2.0;
    o += "<g class=\"truncated\"><line x1=\"30\" y1=\""; num(o, y(step)); o += "\" x2=\"1170\" y2=\""; num(o, y(step));
    o += "\" stroke-width=\"1\" stroke=\"#D96918\"/><text x=\"600\" y=\""; num(o, y(step + 1.0));
    o += "\" fill=\"#D96918\" text-anchor=\"middle\">Additional network events not shown</text></g>\n";
  }
  o += "</svg>\n";
  if (needed) *needed = o.size();
  if (cap == 0) return MSIM_OK;
  if (cap < o.size()) return MSIM_E_RANGE;
  std::memcpy(out, o.data(), o.size());
  return MSIM_OK;
}
