// KAT replay for the restatement: given the golden records written by
// oracle/ref/kat.inc (inputs + reference outputs), recompute every record's
// outputs with the restatement so tests can compare bit for bit.
// TEST INFRASTRUCTURE ONLY.
namespace orc {
static V rd3(const float* p) { return V(p[0], p[1], p[2]); }
static void wr3(float*& o, const V& v) { *o++ = v[0]; *o++ = v[1]; *o++ = v[2]; }
static uint64_t rd_lcg(const float* p) { return (uint64_t)p[0] | ((uint64_t)p[1] << 24); }
static void wr_lcg(float*& o, uint64_t s) { *o++ = (float)(s & 0xFFFFFF); *o++ = (float)((s >> 24) & 0xFFFFFF); }
static uint64_t rd_pcg(const float* p) {
  uint64_t s = 0;
  for (int k = 0; k < 4; ++k) s |= (uint64_t)p[k] << (16 * k);
  return s;
}
static void wr_pcg(float*& o, uint64_t s) {
  for (int k = 0; k < 4; ++k) *o++ = (float)((s >> (16 * k)) & 0xFFFF);
}

// hit t p(3) n(3) [u v]; a miss writes zeros (kat.inc push_rec)
static void wr_rec(float* o, bool hit, const Hit& h, bool uv) {
  *o++ = hit ? 1.f : 0.f;
  *o++ = hit ? h.t : 0;
  wr3(o, hit ? h.p : V(0.f));
  wr3(o, hit ? h.normal : V(0.f));
  if (uv) {
    *o++ = hit ? h.u : 0;
    *o++ = hit ? h.v : 0;
  }
}
// box.h:18-33: six rects in a hitable_list, every second one flipped
static const Hitable* kat_box(Store& St, V p0, V p1) {
  auto mk = [&](int kax, int a0, int a1, float lo0, float hi0, float lo1, float hi1, float kk, bool flip) {
    Rect* q = St.add(new Rect());
    q->kax = kax; q->a0 = a0; q->a1 = a1;
    q->lo0 = lo0; q->hi0 = hi0; q->lo1 = lo1; q->hi1 = hi1; q->k = kk; q->mat = nullptr;
    if (!flip) return (const Hitable*)q;
    Flip* f = St.add(new Flip());
    f->p = q;
    return (const Hitable*)f;
  };
  List* l = St.add(new List());
  l->l = {mk(2, 0, 1, p0.x(), p1.x(), p0.y(), p1.y(), p1.z(), false), mk(2, 0, 1, p0.x(), p1.x(), p0.y(), p1.y(), p0.z(), true),
          mk(1, 0, 2, p0.x(), p1.x(), p0.z(), p1.z(), p1.y(), false), mk(1, 0, 2, p0.x(), p1.x(), p0.z(), p1.z(), p0.y(), true),
          mk(0, 1, 2, p0.y(), p1.y(), p0.z(), p1.z(), p1.x(), false), mk(0, 1, 2, p0.y(), p1.y(), p0.z(), p1.z(), p0.x(), true)};
  return l;
}

// the mesh KAT's scene (tests/golden/kat_mesh.scene, given by oracle_kat_scene): its bvh
// objects in file order; each triangle's material pointer is its index in its bvh
// command + 1 (never dereferenced), as in oracle/ref/kat.inc
static std::unique_ptr<Scene> g_kat_scene;
static std::vector<const Hitable*> g_kat_meshes;
// the world KAT's scene (tests/golden/kat_world.scene): obj 100000 + w is world w; every
// primitive under it carries its position in the depth-first listing of the world's leaves
// (the file's order; a box is its six rects) + 1 as material pointer, as in oracle/ref/kat.inc
struct KatWorld {
  const Hitable* root;
  std::vector<bool> moving;  // per leaf: a moving sphere (its record's u, v are defined as 0)
};
static std::vector<KatWorld> g_kat_worlds;
static void kat_world_tags(const std::string& text) {
  std::map<long long, srr_text::Cmd> by_id;
  for (const auto& c : srr_text::parse(text))
    if (c.at(0) == "obj") by_id[c.i(1)] = c;
  for (int w = 0; by_id.count(100000 + w) && by_id.at(100000 + w).at(2) == "list"; ++w) {
    KatWorld kw;
    kw.root = g_kat_scene->obj.at(100000 + w);
    std::function<void(const Hitable*)> prim = [&](const Hitable* h) {
      const Material* tag = (const Material*)(uintptr_t)(kw.moving.size() + 1);
      if (auto* f = dynamic_cast<const Flip*>(h)) return prim(f->p);
      bool mv = false;
      if (auto* s = dynamic_cast<const Sphere*>(h)) const_cast<Sphere*>(s)->mat = tag;
      else if (auto* m = dynamic_cast<const MovingSphere*>(h)) { const_cast<MovingSphere*>(m)->mat = tag; mv = true; }
      else if (auto* q = dynamic_cast<const Rect*>(h)) const_cast<Rect*>(q)->mat = tag;
      else if (auto* t = dynamic_cast<const Triangle*>(h)) const_cast<Triangle*>(t)->mat = tag;
      else throw std::runtime_error("kat world: a primitive of an unknown class");
      kw.moving.push_back(mv);
    };
    std::function<void(long long)> walk = [&](long long id) {
      const srr_text::Cmd& c = by_id.at(id);
      const std::string& t = c.at(2);
      if (t == "list") for (long long k = 0; k < c.i(3); ++k) walk(c.i(4 + k));
      else if (t == "bvh") for (long long k = 0; k < c.i(5); ++k) walk(c.i(6 + k));
      else if (t == "flip" || t == "translate" || t == "rotate_y" || t == "rotate_x") walk(c.i(3));
      else if (t == "box") {
        const List* l = dynamic_cast<const List*>(dynamic_cast<const Box*>(g_kat_scene->obj.at(id))->l);
        for (const Hitable* k : l->l) prim(k);
      } else prim(g_kat_scene->obj.at(id));
    };
    walk(100000 + w);
    g_kat_worlds.push_back(kw);
  }
}

static void kat_scene(const std::string& text) {
  g_kat_meshes.clear();
  g_kat_worlds.clear();
  g_kat_scene = build(text);
  kat_world_tags(text);
  if (!g_kat_worlds.empty()) return;  // (the world KAT's scene; the mesh KAT's has no list 100000)
  for (const auto& c : srr_text::parse(text))
    if (c.at(0) == "obj" && c.at(2) == "bvh") {
      g_kat_meshes.push_back(g_kat_scene->obj.at(c.i(1)));
      for (long long k = 0; k < c.i(5); ++k) {
        auto* t = const_cast<Triangle*>(dynamic_cast<const Triangle*>(g_kat_scene->obj.at(c.i(6 + k))));
        if (!t) throw std::runtime_error("kat mesh: a bvh child is not a triangle");
        t->mat = (const Material*)(uintptr_t)(k + 1);
      }
    }
}

// the bounce KAT's probe world (oracle/ref/kat.inc KatBounceProbe): the first hit() hands color() the
// record's hit, the second keeps the scattered ray and answers with a white emitter facing it
struct KatBounceProbe : Hitable {
  Hit first;
  const Material* white;
  mutable int calls = 0;
  mutable Ray second;
  bool hit(const Ray& r, float, float, Hit& rec, bool) const override {
    if (calls++ == 0) { rec = first; return true; }
    second = r;
    rec.t = 1;
    rec.p = r.at(1);
    rec.normal = -r.B;
    rec.u = rec.v = 0;
    rec.mat = white;
    return true;
  }
  bool bbox(float, float, AABB&) const override { return false; }
};

// ... and its light list (KatBounceLights): pdf_value is called once per mixture attempt
struct KatBounceLights : List {
  const List* in;
  mutable int calls = 0;
  explicit KatBounceLights(const List* p) : in(p) { l = p->l; }
  float pdf_value(const V& o, const V& v) const override {
    ++calls;
    return in->pdf_value(o, v);
  }
  V random(const V& o) const override { return in->random(o); }
};

static int kat_one(const std::string& name, float* r) {
  float* o;
  if (name == "bounce") {
    // in: l m p n u v o d time depth maxDepth lcg pcg | out: scattered origin dir time colour attempts lcg pcg
    static const ConstTex one(V(1, 1, 1));
    static DiffuseLight white;
    white.emit = &one;
    if (!g_kat_scene) return -1;
    const auto li = g_kat_scene->obj.find(200000 + (long long)r[0]);
    const auto mi = g_kat_scene->mat.find((long long)r[1]);
    if (li == g_kat_scene->obj.end() || mi == g_kat_scene->mat.end() || !dynamic_cast<const List*>(li->second)) return -1;
    KatBounceProbe probe;
    probe.white = &white;
    probe.first.t = 1;
    probe.first.p = rd3(r + 2);
    probe.first.normal = rd3(r + 5);
    probe.first.u = r[8];
    probe.first.v = r[9];
    probe.first.mat = mi->second;
    Scene S;
    S.world = &probe;
    const KatBounceLights lights(dynamic_cast<const List*>(li->second));
    S.lights = &lights;
    R.lcg = rd_lcg(r + 19);
    R.pcg = rd_pcg(r + 21);
    R.inc = 0xda3e39cb94b95bdbULL;
    int depth = (int)r[17];
    const V col = color(S, Ray(rd3(r + 10), rd3(r + 13), r[16]), &depth, (int)r[18]);
    const bool sc = probe.calls == 2;
    o = r + 25;
    *o++ = sc ? 1.f : 0.f;
    wr3(o, sc ? probe.second.A : V(0.f));
    wr3(o, sc ? probe.second.B : V(0.f));
    *o++ = sc ? probe.second.tm : 0;
    wr3(o, col);
    *o++ = (float)lights.calls;  // attempts
    wr_lcg(o, R.lcg);
    wr_pcg(o, R.pcg);
    for (float* c = r + 25; c < o; ++c)  // NaN outputs are canonical in the file (kat.inc kat_bounce_record)
      if (*c != *c) { const uint32_t u = 0x7fc00000u; std::memcpy(c, &u, 4); }
  } else if (name == "mesh") {
    // in: mesh o d tmin tmax is_medium | out: hit t tri p n u v
    const int mi = (int)r[0];
    if (mi < 0 || mi >= (int)g_kat_meshes.size()) return -1;
    Hit h{};
    const bool hit = g_kat_meshes[mi]->hit(Ray(rd3(r + 1), rd3(r + 4)), r[7], r[8], h, r[9] != 0);
    o = r + 10;
    *o++ = hit ? 1.f : 0.f;
    *o++ = hit ? h.t : 0;
    *o++ = hit ? (float)((int)(uintptr_t)h.mat - 1) : -1.f;
    wr3(o, hit ? h.p : V(0.f));
    wr3(o, hit ? h.normal : V(0.f));
    *o++ = hit ? h.u : 0;
    *o++ = hit ? h.v : 0;
  } else if (name == "world") {
    // in: world o d time tmin tmax is_medium | out: hit t obj p n u v, two spare
    const int wi = (int)r[0];
    if (wi < 0 || wi >= (int)g_kat_worlds.size()) return -1;
    Hit h{};
    const bool hit = g_kat_worlds[wi].root->hit(Ray(rd3(r + 1), rd3(r + 4), r[7]), r[8], r[9], h, r[10] != 0);
    const int obj = hit ? (int)(uintptr_t)h.mat - 1 : -1;
    if (hit && g_kat_worlds[wi].moving.at(obj)) h.u = h.v = 0;  // moving_sphere::hit leaves u, v unset: defined as 0
    o = r + 11;
    *o++ = hit ? 1.f : 0.f;
    *o++ = hit ? h.t : 0;
    *o++ = (float)obj;
    wr3(o, hit ? h.p : V(0.f));
    wr3(o, hit ? h.normal : V(0.f));
    *o++ = hit ? h.u : 0;
    *o++ = hit ? h.v : 0;
    *o++ = 0;
    *o++ = 0;
  } else if (name == "erf") {
    o = r + 1;
    *o++ = Erf(r[0]);
    *o++ = ErfInv(r[0]);
  } else if (name == "beckmann11") {
    float sx, sy;
    Beckmann::Sample11(r[0], r[1], r[2], &sx, &sy);
    r[3] = sx;
    r[4] = sy;
  } else if (name == "beckmann_dist") {
    Beckmann d;
    d.ax = Beckmann::RoughnessToAlpha(r[0]);
    d.ay = Beckmann::RoughnessToAlpha(r[1]);
    V wo = rd3(r + 2);
    V wh = d.Sample_wh(wo, r[5], r[6]);
    o = r + 7;
    *o++ = d.ax;
    *o++ = d.ay;
    wr3(o, wh);
    *o++ = d.D(wh);
    *o++ = d.G(wo, wh);
    *o++ = d.Pdf(wo, wh);
    *o++ = d.Lambda(wo);
  } else if (name == "beckmann_pdf") {
    ConstTex one(V(1));
    BeckmannMat m(&one, r[0], r[1]);
    V n = rd3(r + 2), wo = rd3(r + 5);
    BeckmannPdf bp(&m.dist, n);
    R.pcg = rd_pcg(r + 8);
    R.inc = 0xda3e39cb94b95bdbULL;
    V wi = bp.generate(wo);
    float val = bp.value(wo, wi);
    Hit h;
    h.normal = n;
    float sp = m.scattering_pdf(Ray(V(0.f), wo), h, Ray(V(0.f), wi));
    o = r + 12;
    wr3(o, wi);
    *o++ = val;
    *o++ = sp;
    wr_pcg(o, R.pcg);
  } else if (name == "cosine_pdf" || name == "orennayar_pdf") {
    ConstTex one(V(1));
    OrenNayar on(&one, r[0]);
    V n = rd3(r + 1), wo = rd3(r + 4);
    std::unique_ptr<Pdf> p(name == "cosine_pdf" ? (Pdf*)new CosinePdf(n) : (Pdf*)new OrenNayarPdf(n, on.A, on.B));
    R.lcg = rd_lcg(r + 7);
    V d = p->generate(wo);
    V w2 = rd3(r + 16);
    o = r + 9;
    *o++ = on.A;
    *o++ = on.B;
    wr3(o, d);
    *o++ = p->value(wo, d);
    *o++ = p->value(wo, w2);
    o += 3;
    wr_lcg(o, R.lcg);
  } else if (name == "dielectric" || name == "metal") {
    std::unique_ptr<Material> m;
    if (name == "dielectric") {
      auto* q = new Dielectric();
      q->ref_idx = r[0];
      m.reset(q);
    } else {
      auto* q = new Metal();
      q->albedo = V(0.5f);
      q->fuzz = (r[0] < 1) ? r[0] : 1;
      m.reset(q);
    }
    Hit h;
    h.normal = rd3(r + 4);
    h.p = V(1, 2, 3);
    Scatter s;
    R.lcg = rd_lcg(r + 7);
    m->scatter(Ray(V(0.f), rd3(r + 1), 0.25f), h, s);
    o = r + 9;
    wr3(o, s.specular_ray.B);
    wr_lcg(o, R.lcg);
  } else if (name == "triangle") {
    Triangle t(rd3(r), rd3(r + 3), rd3(r + 6), nullptr);
    t.uv0 = V(0.1f, 0.2f, 0);
    t.uv1 = V(0.7f, 0.1f, 0);
    t.uv2 = V(0.3f, 0.9f, 0);
    t.n0 = t.n1 = t.n2 = t.normal;
    Hit h{};
    bool hit = t.hit(Ray(rd3(r + 9), rd3(r + 12)), 0.001f, FLT_MAX, h, r[15] != 0);
    o = r + 16;
    *o++ = hit ? 1.f : 0.f;
    *o++ = hit ? h.t : 0;
    *o++ = hit ? h.u : 0;
    *o++ = hit ? h.v : 0;
    wr3(o, hit ? h.normal : V(0.f));
    wr3(o, hit ? h.p : V(0.f));
  } else if (name == "aabb") {
    AABB b{rd3(r), rd3(r + 3)};
    r[14] = b.hit(Ray(rd3(r + 6), rd3(r + 9)), r[12], r[13]) ? 1.f : 0.f;
  } else if (name == "camera") {
    Camera cam(rd3(r), rd3(r + 3), V(0, 1, 0), r[6], r[7], r[8], r[9], 0.0f, 1.0f);
    R.lcg = rd_lcg(r + 12);
    Ray ry = cam.get_ray(r[10], r[11]);
    o = r + 14;
    wr3(o, ry.A);
    wr3(o, ry.B);
    *o++ = ry.tm;
    wr_lcg(o, R.lcg);
  } else if (name == "lights") {
    Rect rect;
    rect.kax = 1; rect.a0 = 0; rect.a1 = 2;
    rect.lo0 = 213; rect.hi0 = 343; rect.lo1 = 227; rect.hi1 = 332; rect.k = 554; rect.mat = nullptr;
    Flip fr;
    fr.p = &rect;
    Sphere sph(V(278, 700, 280), 50, nullptr);
    V org = rd3(r);
    R.lcg = rd_lcg(r + 3);
    V d1 = fr.random(org);
    float p1 = fr.pdf_value(org, d1);
    V d2 = sph.random(org);
    float p2 = sph.pdf_value(org, d2);
    o = r + 5;
    wr3(o, d1);
    *o++ = p1;
    wr3(o, d2);
    *o++ = p2;
    wr_lcg(o, R.lcg);
  } else if (name == "merl" || name == "merl_same") {
    // brdf.h:17-61, 109-154, 190-214 restated (double precision, reference order);
    // merl_same: brdfmaterial::scatter's out == in queries (material.h:214-231)
    static std::vector<double> tab = [] {
      std::vector<double> t(3 * 90 * 90 * 180);
      for (size_t k = 0; k < t.size(); ++k)
        t[k] = (k % 97 == 0) ? -1.0 : (double)(((unsigned long long)k * 2654435761ULL) % 1000003ULL) / 1000.0;
      return t;
    }();
    const double PI = 3.1415926535897932384626433832795;
    auto norm = [](double* v) {
      double len = std::sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]);
      for (int k = 0; k < 3; ++k) v[k] = v[k] / len;
    };
    // the reference's build calls glibc's separate cos() and sin() here (FMA ifunc
    // variants) but merges each input angle's sin and cos into one sincos() (a
    // non-FMA build): spelled out, so this TU's optimiser cannot choose otherwise
    static double (*volatile cos_f)(double) = ::cos;
    static double (*volatile sin_f)(double) = ::sin;
    auto rot = [](const double* v, const double* ax, double ang, double* o) {
      double c = cos_f(ang), sn = sin_f(ang);
      for (int k = 0; k < 3; ++k) o[k] = v[k] * c;
      double t = (ax[0] * v[0] + ax[1] * v[1] + ax[2] * v[2]) * (1.0 - c);
      for (int k = 0; k < 3; ++k) o[k] += ax[k] * t;
      double x[3] = {ax[1] * v[2] - ax[2] * v[1], ax[2] * v[0] - ax[0] * v[2], ax[0] * v[1] - ax[1] * v[0]};
      for (int k = 0; k < 3; ++k) o[k] += x[k] * sn;
    };
    double ti = r[0], fi = r[1], to = r[2], fo = r[3];
    double sti, cti, sfi, cfi, sto, cto, sfo, cfo;
    ::sincos(ti, &sti, &cti);
    ::sincos(fi, &sfi, &cfi);
    ::sincos(to, &sto, &cto);
    ::sincos(fo, &sfo, &cfo);
    double in[3] = {sti * cfi, sti * sfi, cti};
    double ou[3] = {sto * cfo, sto * sfo, cto};
    double h[3] = {(in[0] + ou[0]) / 2.0, (in[1] + ou[1]) / 2.0, (in[2] + ou[2]) / 2.0};
    norm(in);
    norm(h);
    double th = std::acos(h[2]), fh = std::atan2(h[1], h[0]);
    const double bn[3] = {0, 1, 0}, nz[3] = {0, 0, 1};
    double tmp[3], df[3];
    rot(in, nz, -fh, tmp);
    rot(tmp, bn, -th, df);
    double td = std::acos(df[2]), fd = std::atan2(df[1], df[0]);
    int ih = 0;
    if (th > 0.0) {
      ih = (int)std::sqrt(((th / (PI / 2.0)) * 90) * 90);
      ih = ih < 0 ? 0 : (ih >= 90 ? 89 : ih);
    }
    int id = int(td / (PI * 0.5) * 90);
    id = id < 0 ? 0 : (id < 89 ? id : 89);
    double f = fd < 0.0 ? fd + PI : fd;
    int ip = int(f / PI * 360 / 2);
    ip = ip < 0 ? 0 : (ip < 179 ? ip : 179);
    int cell = ip + id * 180 + ih * 180 * 90;
    const int nc = 90 * 90 * 180;
    double rgb[3] = {tab[cell] * (1.0 / 1500.0), tab[cell + nc] * (1.15 / 1500.0), tab[cell + 2 * nc] * (1.66 / 1500.0)};
    o = r + 4;
    *o++ = (float)cell;
    *o++ = (float)th;
    *o++ = (float)fh;
    *o++ = (float)td;
    *o++ = (float)fd;
    for (double d : rgb) {
      unsigned long long u;
      std::memcpy(&u, &d, 8);
      *o++ = (float)(u & 0xFFFFFF);
      *o++ = (float)((u >> 24) & 0xFFFFFF);
      *o++ = (float)(u >> 48);
    }
  } else if (name == "light_list") {
    Rect rect;
    rect.kax = 1; rect.a0 = 0; rect.a1 = 2;
    rect.lo0 = 213; rect.hi0 = 343; rect.lo1 = 227; rect.hi1 = 332; rect.k = 554; rect.mat = nullptr;
    Flip fr;
    fr.p = &rect;
    Sphere sph(V(278, 700, 280), 50, nullptr);
    Triangle tr(V(150, 500, 150), V(400, 520, 180), V(260, 540, 420), nullptr);
    tr.n0 = tr.n1 = tr.n2 = tr.normal;
    List hl;
    hl.l = {&fr, &sph, &tr};
    V org = rd3(r);
    R.lcg = rd_lcg(r + 3);
    V d1 = hl.random(org);
    float p1 = hl.pdf_value(org, d1);
    V d2 = tr.random(org);
    float p2 = tr.pdf_value(org, d2);
    o = r + 5;
    wr3(o, d1);
    *o++ = p1;
    wr3(o, d2);
    *o++ = p2;
    wr_lcg(o, R.lcg);
  } else if (name == "sphere") {
    Sphere s(rd3(r), r[3], nullptr);
    Hit h{};
    bool hit = s.hit(Ray(rd3(r + 4), rd3(r + 7)), r[10], r[11], h, false);
    wr_rec(r + 12, hit, h, true);
  } else if (name == "moving_sphere") {
    MovingSphere s;
    s.c0 = rd3(r); s.c1 = rd3(r + 3); s.t0 = r[6]; s.t1 = r[7]; s.radius = r[8]; s.mat = nullptr;
    Hit h{};
    bool hit = s.hit(Ray(rd3(r + 9), rd3(r + 12), r[15]), r[16], r[17], h, false);
    wr_rec(r + 18, hit, h, false);
  } else if (name == "rect") {
    const int kind = (int)r[0];
    Rect q;
    q.kax = kind == 0 ? 2 : (kind == 1 ? 1 : 0);
    q.a0 = kind == 2 ? 1 : 0;
    q.a1 = kind == 0 ? 1 : 2;
    q.lo0 = r[2]; q.hi0 = r[3]; q.lo1 = r[4]; q.hi1 = r[5]; q.k = r[6]; q.mat = nullptr;
    Flip f;
    f.p = &q;
    const Hitable* hh = r[1] != 0 ? (const Hitable*)&f : (const Hitable*)&q;
    Hit h{};
    bool hit = hh->hit(Ray(rd3(r + 7), rd3(r + 10)), r[13], r[14], h, false);
    o = r + 15;
    *o++ = hit ? 1.f : 0.f;
    *o++ = hit ? h.t : 0;
    *o++ = hit ? h.u : 0;
    *o++ = hit ? h.v : 0;
    wr3(o, hit ? h.p : V(0.f));
    wr3(o, hit ? h.normal : V(0.f));
  } else if (name == "box") {
    Store St;
    const Hitable* bx = kat_box(St, rd3(r), rd3(r + 3));
    Hit h{};
    bool hit = bx->hit(Ray(rd3(r + 6), rd3(r + 9)), r[12], r[13], h, false);
    wr_rec(r + 14, hit, h, true);
  } else if (name == "xform") {
    Store St;
    const Hitable* hh = r[0] == 0 ? (const Hitable*)St.add(new Sphere(rd3(r + 1), r[4], nullptr)) : kat_box(St, rd3(r + 1), rd3(r + 4));
    for (int l = 2; l >= 0; --l) {  // the wrappers are listed outermost first
      const float* w = r + 7 + 4 * l;
      const int kind = (int)w[0];
      if (kind == 1) {
        auto* t = St.add(new Translate());
        t->p = hh;
        t->off = rd3(w + 1);
        hh = t;
      } else if (kind == 2 || kind == 3) {
        hh = St.add(new Rotate(hh, w[1], kind == 2));
      } else if (kind == 4) {
        auto* f = St.add(new Flip());
        f->p = hh;
        hh = f;
      }
    }
    Hit h{};
    bool hit = hh->hit(Ray(rd3(r + 19), rd3(r + 22)), r[25], r[26], h, false);
    wr_rec(r + 27, hit, h, false);
  } else if (name == "medium") {
    Store St;
    Medium md;
    md.boundary = r[0] == 0 ? (const Hitable*)St.add(new Sphere(rd3(r + 1), r[4], nullptr)) : kat_box(St, rd3(r + 1), rd3(r + 4));
    md.density = r[7];
    md.phase = nullptr;
    Hit h{};
    R.lcg = rd_lcg(r + 16);
    bool hit = md.hit(Ray(rd3(r + 8), rd3(r + 11)), r[14], r[15], h, false);
    o = r + 18;
    *o++ = hit ? 1.f : 0.f;
    *o++ = hit ? h.t : 0;
    wr_lcg(o, R.lcg);
  } else if (name == "isotropic") {
    static const ConstTex cA(V(0.2f, 0.3f, 0.1f)), cB(V(0.9f, 0.9f, 0.9f));
    CheckerTex alb;
    alb.even = &cA;
    alb.odd = &cB;
    Isotropic iso;
    iso.albedo = &alb;
    Hit h{};
    h.p = rd3(r);
    h.u = 0.25f;
    h.v = 0.75f;
    Scatter s;
    R.lcg = rd_lcg(r + 3);
    iso.scatter(Ray(V(0.f), V(1, 0, 0)), h, s);
    o = r + 5;
    wr3(o, s.specular_ray.B);
    wr3(o, s.attenuation);
    wr_lcg(o, R.lcg);
  } else if (name == "texture_checker") {
    static const ConstTex cA(V(0.2f, 0.3f, 0.1f)), cB(V(0.9f, 0.9f, 0.9f)), cC(V(0.1f, 0.5f, 0.8f)), cD(V(0.6f, 0.1f, 0.4f));
    CheckerTex ab, cd, nested;
    ab.even = &cA; ab.odd = &cB;
    cd.even = &cC; cd.odd = &cD;
    nested.even = &ab; nested.odd = &cd;
    o = r + 4;
    wr3(o, (r[0] != 0 ? nested : ab).value(0.f, 0.f, rd3(r + 1)));
  } else if (name == "texture_noise") {
    NoiseTex nt;
    nt.scale = r[0];
    o = r + 4;
    wr3(o, nt.value(0.f, 0.f, rd3(r + 1)));
  } else if (name == "texture_image") {
    static const ImageTex im = [] {
      ImageTex t;
      t.nx = 7;
      t.ny = 5;
      t.px = srr_text::gen_image(7, 5, 7u, 0);
      return t;
    }();
    o = r + 2;
    wr3(o, im.value(r[0], r[1], V(0.f)));
  } else {
    return -1;
  }
  return 0;
}
}  // namespace orc

// the scene text the `mesh` KAT replays over (call before oracle_kat("mesh", ...))
extern "C" int oracle_kat_scene(const char* text) {
  try {
    orc::kat_scene(text);
  } catch (const std::exception& e) {
    orc::g_err = e.what();
    return -1;
  }
  return 0;
}

extern "C" int oracle_kat(const char* name, int n, int width, float* records) {
  std::string nm(name);
  for (int q = 0; q < n; ++q)
    if (orc::kat_one(nm, records + (size_t)q * width) != 0) {
      orc::g_err = "unknown kat " + nm;
      return -1;
    }
  return 0;
}
