#!/usr/bin/env python3
"""Write the `.pbrt` file that makes rs_pbrt build one of this repo's test scenes, so that a machine with cargo can produce
reference fixtures for the oracle (rust_shim/refdump.rs -> tools/ref_to_npz.py -> tests/test_reference_fixtures.py).

    python tools/export_pbrt.py            # (re)writes tests/golden/ref_scenes/*.pbrt and their rays.bin

Covers what rs_pbrt's own parser + API produce for: triangle meshes in world space (with uv / normals), the materials that carry a
"pbrt" string (rs_pbrt_amd/scenes.py: matte, plastic, mirror, glass, metal, substrate — colour / roughness / bump parameters may be
textures), the procedural texture classes (constant, scale, mix, checkerboard, dots, fbm, wrinkled, windy, marble; image textures
are left out: an 8-bit file would not carry the generator's float texels), diffuse area lights, point lights, a LookAt + perspective
camera, box filter, every sampler the library takes (Sobol', Halton, random, 02sequence, stratified, maxmindist), homogeneous media
with MediumInterface per shape, `path` / `volpath`.

Texture directives follow make_texture (api.rs:1039-1600), quirks included: the float namespace has no checkerboard and no marble
(":1175 TODO", ":1263 TODO"); `DotsTexture::new(mapping, inside, outside)` is called with the arguments of a constructor declared
`(mapping, outside_dot, inside_dot)` (api.rs:1228, :1531 vs dots.rs:19-23), so the directive's "inside" is the record's outside;
a 3-D mapping's world_to_texture is the CTM at the directive (IdentityMapping3D::new(tex_2_world), :1242)."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))


def f(v):
    return " ".join("%.9g" % float(np.float32(x)) for x in np.asarray(v).reshape(-1))


def sampler_directive(sampler, spp, dimensions=4, strat=(4, 4), jitter=True):
    """make_sampler (api.rs:1690-1720): the parameters each sampler reads"""
    if sampler in ("sobol", "halton", "random"):
        return 'Sampler "%s" "integer pixelsamples" [%d]' % (sampler, spp)
    if sampler == "stratified":
        return 'Sampler "stratified" "integer xsamples" [%d] "integer ysamples" [%d] "bool jitter" ["%s"] "integer dimensions" [%d]' % (
            strat[0], strat[1], "true" if jitter else "false", dimensions)
    return 'Sampler "%s" "integer pixelsamples" [%d] "integer dimensions" [%d]' % (sampler, spp, dimensions)   # 02sequence / lowdiscrepancy / maxmindist


def texture_directives(sb):
    """Texture directives for the builder's texture records, children first; float or spectrum by how each record is used"""
    from rs_pbrt_amd import abi
    T = sb.textures
    kind_of = {}   # index -> "float" | "spectrum"

    def mark(i, ty):
        assert kind_of.get(i, ty) == ty, "texture %d is used both as a float and as a spectrum texture: declare it twice" % i
        if i in kind_of:
            return
        kind_of[i] = ty
        k = int(T[i]["kind"])
        if k in (abi.TEX_SCALE, abi.TEX_MIX, abi.TEX_CHECKERBOARD, abi.TEX_DOTS):
            mark(int(T[i]["tex1"]), ty); mark(int(T[i]["tex2"]), ty)
        if k == abi.TEX_MIX:
            mark(int(T[i]["tex3"]), "float")
    from rs_pbrt_amd import scenes as _sc
    for m in sb.materials:
        for ref, ty in _sc.material_texrefs(m):
            mark(ref.index, ty)
    for fl in sb.meshes:
        for a in (fl[4], fl[5]):
            if a:
                mark(int(a) - 1, "float")

    def child(name, i, ty):   # a constant child is written inline, anything else by name
        if int(T[i]["kind"]) == abi.TEX_CONSTANT:
            return '"rgb %s" [%s]' % (name, f(T[i]["value"])) if ty == "spectrum" else '"float %s" [%.9g]' % (name, float(T[i]["value"][0]))
        return '"texture %s" "tex%d"' % (name, i)

    def mapping2d(t):
        mk = int(t["mapping"])
        if mk == abi.MAP_UV:
            return '"string mapping" ["uv"] "float uscale" [%.9g] "float vscale" [%.9g] "float udelta" [%.9g] "float vdelta" [%.9g]' % tuple(float(x) for x in t["map"][:4])
        if mk == abi.MAP_PLANAR:
            return '"string mapping" ["planar"] "vector v1" [%s] "vector v2" [%s] "float udelta" [%.9g] "float vdelta" [%.9g]' % (
                f(t["map"][:3]), f(t["map"][3:6]), float(t["map"][6]), float(t["map"][7]))
        return '"string mapping" ["%s"]' % {abi.MAP_SPHERICAL: "spherical", abi.MAP_CYLINDRICAL: "cylindrical"}[mk]

    out, files = [], []
    for i in sorted(kind_of):   # records are appended children first (SceneBuilder), so index order is declaration order
        t, ty = T[i], kind_of[i]
        k = int(t["kind"])
        head = 'Texture "tex%d" "%s"' % (i, ty)
        uses_ctm = k in (abi.TEX_FBM, abi.TEX_WRINKLED, abi.TEX_WINDY, abi.TEX_MARBLE) or int(t["mapping"]) in (abi.MAP_SPHERICAL, abi.MAP_CYLINDRICAL)
        if k == abi.TEX_CONSTANT:
            line = head + ' "constant" ' + ('"rgb value" [%s]' % f(t["value"]) if ty == "spectrum" else '"float value" [%.9g]' % float(t["value"][0]))
        elif k == abi.TEX_SCALE:
            line = head + ' "scale" %s %s' % (child("tex1", int(t["tex1"]), ty), child("tex2", int(t["tex2"]), ty))
        elif k == abi.TEX_MIX:
            line = head + ' "mix" %s %s %s' % (child("tex1", int(t["tex1"]), ty), child("tex2", int(t["tex2"]), ty), child("amount", int(t["tex3"]), "float"))
        elif k == abi.TEX_CHECKERBOARD:
            assert ty == "spectrum", "rs_pbrt has no float checkerboard (api.rs:1175)"
            line = head + ' "checkerboard" "integer dimension" [2] %s %s %s' % (child("tex1", int(t["tex1"]), ty), child("tex2", int(t["tex2"]), ty), mapping2d(t))
        elif k == abi.TEX_DOTS:   # record: tex1 = outside_dot, tex2 = inside_dot; the API hands "inside" to the outside_dot slot
            line = head + ' "dots" %s %s %s' % (child("inside", int(t["tex1"]), ty), child("outside", int(t["tex2"]), ty), mapping2d(t))
        elif k in (abi.TEX_FBM, abi.TEX_WRINKLED):
            line = head + ' "%s" "integer octaves" [%d] "float roughness" [%.9g]' % ("fbm" if k == abi.TEX_FBM else "wrinkled", int(t["octaves"]), float(t["omega"]))
        elif k == abi.TEX_WINDY:
            line = head + ' "windy"'
        elif k == abi.TEX_MARBLE:
            assert ty == "spectrum", "rs_pbrt has no float marble (api.rs:1263)"
            line = head + ' "marble" "integer octaves" [%d] "float roughness" [%.9g] "float scale" [%.9g] "float variation" [%.9g]' % (
                int(t["octaves"]), float(t["omega"]), float(t["scale"]), float(t["variation"]))
        elif k == abi.TEX_IMAGE:   # CreateImage{Float,Spectrum}Texture (api.rs:1095-1170, :1320-1405): every parameter spelled out
            src = sb.image_src.get(int(t["image"]))
            assert src is not None and not src["gamma"] and src["channels"] == (1 if ty == "float" else 3), \
                "exporter: an image texture needs an 8-bit source (SceneBuilder.image_texture_u8) without gamma: the file must carry the generator's texels"
            files.append(("img%d.png" % int(t["image"]), src["u8"]))
            line = head + ' "imagemap" "string filename" ["%s_img%d.png"] "bool gamma" ["false"] "float scale" [%.9g] "bool trilinear" ["%s"] "float maxanisotropy" [%.9g] "string wrap" ["%s"] %s' % (
                "%s", int(t["image"]), src["scale"], "true" if int(t["trilinear"]) else "false", float(t["max_aniso"]),
                {abi.WRAP_REPEAT: "repeat", abi.WRAP_BLACK: "black", abi.WRAP_CLAMP: "clamp"}[int(t["wrap"])], mapping2d(t))
        else:
            raise NotImplementedError("exporter: texture kind %d" % k)
        if uses_ctm:   # the Transform directive reads its 16 numbers column by column (bin/rs_pbrt.rs:729-748)
            w = np.asarray(t["world_to_texture"], np.float32).reshape(4, 4)
            out += ["TransformBegin", "  Transform [%s]" % f(w.T), "  " + line, "TransformEnd"]
        else:
            out.append(line)
    return out, files


def integrator_directive(integrator, max_depth, direct_strategy="all", ao_samples=64, ao_cos_sample=True):
    """make_integrator (api.rs:246-435): the parameters each integrator reads"""
    if integrator == "directlighting":
        return 'Integrator "directlighting" "integer maxdepth" [%d] "string strategy" ["%s"]' % (max_depth, direct_strategy)
    if integrator == "ao":
        return 'Integrator "ambientocclusion" "integer nsamples" [%d] "bool cossample" ["%s"]' % (ao_samples, "true" if ao_cos_sample else "false")
    return 'Integrator "%s" "integer maxdepth" [%d]' % (integrator, max_depth)


def export(sc, path, look_at, fov, xres, yres, spp, max_depth=5, sampler="sobol", integrator="path", **kw):
    integ_kw = {k: kw.pop(k) for k in ("direct_strategy", "ao_samples", "ao_cos_sample") if k in kw}
    cam_kw = {k: kw.pop(k) for k in ("look_at_end", "camera_times", "shutter", "lens_radius", "focal_distance", "mirror_x") if k in kw}
    filt = kw.pop("filter", None)   # ("gaussian", (xwidth, ywidth), alpha): GaussianFilter::create (filters/gaussian.rs); None = the box filter the library's default table restates
    sampler_kw = kw
    sb = sc.builder
    assert sb is not None, "the scene was not made by a SceneBuilder"
    cam_xf = ["LookAt %s  %s  %s" % tuple(f(v) for v in look_at)]
    cam_par = ""
    if cam_kw.get("mirror_x"):
        cam_xf = ["Scale -1 1 1"] + cam_xf
    if cam_kw.get("look_at_end") is not None:   # a moving camera: the CTM's two slots (api.rs active_transform_bits), AnimatedTransform::new in make_camera
        t0, t1 = cam_kw.get("camera_times", (0.0, 1.0))
        so, sc_ = cam_kw.get("shutter", (0.0, 1.0))
        cam_xf = ["TransformTimes %.9g %.9g" % (t0, t1), "ActiveTransform StartTime", cam_xf[0], "ActiveTransform EndTime",
                  "LookAt %s  %s  %s" % tuple(f(v) for v in cam_kw["look_at_end"]), "ActiveTransform All"]
        cam_par += ' "float shutteropen" [%.9g] "float shutterclose" [%.9g]' % (so, sc_)
    if cam_kw.get("lens_radius"):
        cam_par += ' "float lensradius" [%.9g] "float focaldistance" [%.9g]' % (cam_kw["lens_radius"], cam_kw.get("focal_distance", 1e6))
    out = ["# generated by tools/export_pbrt.py from rs_pbrt_amd/scenes.py — do not edit"] + cam_xf + [
           'Camera "perspective" "float fov" [%.9g]%s' % (fov, cam_par),
           sampler_directive(sampler, spp, **sampler_kw),
           integrator_directive(integrator, max_depth, **integ_kw),
           ('PixelFilter "box" "float xwidth" [0.5] "float ywidth" [0.5]' if filt is None else
            'PixelFilter "%s" "float xwidth" [%.9g] "float ywidth" [%.9g] "float alpha" [%.9g]' % (filt[0], filt[1][0], filt[1][1], filt[2])),
           'Film "image" "integer xresolution" [%d] "integer yresolution" [%d] "string filename" ["ref.png"]' % (xres, yres),
           "WorldBegin"]
    for k, md in enumerate(sb.media):   # MakeNamedMedium (api.rs:953-1037): sigma_a / sigma_s are already scaled in the builder
        out.append('MakeNamedMedium "medium%d" "string type" ["homogeneous"] "rgb sigma_a" [%s] "rgb sigma_s" [%s] "float g" [%.9g] "float scale" [1]' % (
            k + 1, f(md["sigma_a"]), f(md["sigma_s"]), float(md["g"])))
    tex, files = texture_directives(sb)
    stem = os.path.splitext(os.path.basename(path))[0]
    out += [l.replace("%s_img", stem + "_img") if '"imagemap"' in l else l for l in tex]   # image files sit next to the scene file (api.rs:1381-1388)
    from imgio import write_png_u8
    for name, u8 in files:
        write_png_u8(os.path.join(os.path.dirname(path), "%s_%s" % (stem, name)), u8)
    from rs_pbrt_amd import abi as _abi

    def mesh_block(m, indent=""):
        blk = []
        flags, mat, emit = sb.meshes[m], sb.mesh_material[m], sb.mesh_emit[m]
        text = 'Material ""' if mat == _abi.NO_MATERIAL else sb.materials[mat].get("pbrt")   # Material "" / "none": no BSDF (a medium boundary)
        assert text, "material %d has no pbrt directive (textured parameter?)" % mat
        if isinstance(text, tuple):   # a mix of the two named materials declared before the shapes
            text = 'Material "mix" "string namedmaterial1" ["mat%d_1"] "string namedmaterial2" ["mat%d_2"] %s' % (mat, mat, text[3])
        blk.append(indent + "AttributeBegin")
        if flags[6] or flags[7]:   # the shape's MediumInterface: inside, outside ("" = no medium)
            blk.append(indent + '  MediumInterface "%s" "%s"' % ("medium%d" % flags[6] if flags[6] else "", "medium%d" % flags[7] if flags[7] else ""))
        if emit is not None:
            blk.append(indent + '  AreaLightSource "diffuse" "rgb L" [%s] "bool twosided" ["%s"]' % (f(emit[0]), "true" if emit[1] else "false"))
        blk.append(indent + "  " + text)
        if flags[3]:
            blk.append(indent + "  ReverseOrientation")
        first = sum(len(p) for p in sb.P[:m])
        idx = sb.tris[m].astype(np.int64) - first
        extra = ""
        if flags[0]:
            extra += ' "normal N" [%s]' % f(sb.N[m])
        if flags[2]:
            extra += ' "float uv" [%s]' % f(sb.UV[m])
        for key, a in (("alpha", flags[4]), ("shadowalpha", flags[5])):   # float textures by name (api.rs:1920-1965)
            if a:
                extra += ' "texture %s" "tex%d"' % (key, a - 1)
        blk.append(indent + '  Shape "trianglemesh" "integer indices" [%s] "point P" [%s]%s' % (" ".join(str(int(i)) for i in idx.reshape(-1)), f(sb.P[m]), extra))
        blk.append(indent + "AttributeEnd")
        return blk

    import re
    for k, m in enumerate(sb.materials):   # MakeNamedMaterial "name" "string type" ["matte"] <the parameters of the Material directive> (api.rs:2740-2770)
        if isinstance(m.get("pbrt"), tuple):
            for side in (1, 2):
                mm = re.match(r'Material "(\w+)" (.*)$', m["pbrt"][side])
                out.append('MakeNamedMaterial "mat%d_%d" "string type" ["%s"] %s' % (k, side, mm.group(1), mm.group(2)))
    # ObjectBegin / ObjectEnd first (their order does not reach render_options.primitives), then the top-level declarations in order.
    # An instance's transform is written as one Transform directive, so rs_pbrt derives m_inv by Matrix4x4::inverse — the scene must
    # have been built with Transform(m) (scenes.py computes the same Gauss-Jordan inverse), not with a product of (m, m_inv) pairs.
    names = {v: k for k, v in sb.objects.items()}
    for o in sorted(names):
        out.append('ObjectBegin "%s"' % names[o])
        for m in range(len(sb.meshes)):
            if sb.mesh_object[m] == o:
                out += mesh_block(m, "  ")
        out.append("ObjectEnd")
    def sphere_block(k, what="sphere"):
        """Shape "sphere" (or, ABI 27, "disk" / "cylinder") under its own CTM: one Transform directive, so rs_pbrt derives world_to_object by Matrix4x4::inverse — the builder's
        Transform must be Transform(m); an area light's AreaLightSource comes before the shape (api.rs make_shapes / pbrt_shape)"""
        _rec, mat, emit, prm = {"sphere": sb.spheres, "disk": sb.disks, "cylinder": sb.cylinders}[what][k]
        from rs_pbrt_amd import scenes as _sc
        xf = prm["xf"]
        assert np.array_equal(np.asarray(xf.m_inv, np.float32), np.asarray(_sc.Transform(xf.m).m_inv, np.float32)), "sphere transform was not built as Transform(m)"
        text = 'Material ""' if mat == _abi.NO_MATERIAL else sb.materials[mat].get("pbrt")
        assert text, "material %d has no pbrt directive (textured parameter?)" % mat
        if isinstance(text, tuple):
            text = 'Material "mix" "string namedmaterial1" ["mat%d_1"] "string namedmaterial2" ["mat%d_2"] %s' % (mat, mat, text[3])
        blk = ["AttributeBegin"]
        mi, mo = int(_rec["medium_inside"]), int(_rec["medium_outside"])
        if mi or mo:
            blk.append('  MediumInterface "%s" "%s"' % ("medium%d" % mi if mi else "", "medium%d" % mo if mo else ""))
        if emit is not None:
            blk.append('  AreaLightSource "diffuse" "rgb L" [%s] "bool twosided" ["%s"]' % (f(emit[0]), "true" if emit[1] else "false"))
        if what == "disk":
            shape = '  Shape "disk" "float height" [%s] "float radius" [%s] "float innerradius" [%s] "float phimax" [%s]' % (
                f(prm["height"]), f(prm["radius"]), f(prm["innerradius"]), f(prm["phimax"]))
        else:
            shape = '  Shape "%s" "float radius" [%s] "float zmin" [%s] "float zmax" [%s] "float phimax" [%s]' % (
                what, f(prm["radius"]), f(prm["zmin"]), f(prm["zmax"]), f(prm["phimax"]))
        blk += ["  " + text, "  Transform [%s]" % f(np.asarray(xf.m, np.float32).reshape(4, 4).T), shape, "AttributeEnd"]
        return blk

    for what, k in sb.decl:
        if what == "mesh":
            out += mesh_block(k)
        elif what in ("sphere", "disk", "cylinder"):
            out += sphere_block(k, what)
        else:
            obj, xf, xf_end, _times = sb.instances[k]
            from rs_pbrt_amd import scenes as _sc
            assert np.array_equal(np.asarray(xf.m_inv, np.float32), np.asarray(_sc.Transform(xf.m).m_inv, np.float32)), "instance transform was not built as Transform(m)"
            if xf_end is None:
                out += ["TransformBegin", "  Transform [%s]" % f(np.asarray(xf.m, np.float32).reshape(4, 4).T), '  ObjectInstance "%s"' % names[obj], "TransformEnd"]
            else:   # a MOVING instance: the CTM's two slots set apart (api.rs active_transform_bits), pbrt_object_instance makes AnimatedTransform(ctm[0], start, ctm[1], end)
                assert np.array_equal(np.asarray(xf_end.m_inv, np.float32), np.asarray(_sc.Transform(xf_end.m).m_inv, np.float32)), "instance end key was not built as Transform(m)"
                out += ["TransformBegin", "  ActiveTransform StartTime", "  Transform [%s]" % f(np.asarray(xf.m, np.float32).reshape(4, 4).T),
                        "  ActiveTransform EndTime", "  Transform [%s]" % f(np.asarray(xf_end.m, np.float32).reshape(4, 4).T), "  ActiveTransform All",
                        '  ObjectInstance "%s"' % names[obj], "TransformEnd"]
    # point lights after the shapes: the builder lists Scene.lights as area lights (declaration order) then the others
    for lt in sb.delta_lights:
        from rs_pbrt_amd import abi
        if lt["kind"] == abi.LIGHT_POINT:
            out.append('LightSource "point" "point from" [%s] "rgb I" [%s]' % (f(lt["p"][:3]), f(lt["L"])))
        elif lt["kind"] == abi.LIGHT_INFINITE:   # constant radiance only: the 1x1 map InfiniteAreaLight::new makes of L (api.rs:918-950); a file would have to be .hdr
            env = sb.envmaps[int(lt["prim"])]
            assert env["width"] == env["height"] == 1 and np.array_equal(np.asarray(lt["p"][:9], np.float32).reshape(3, 3), np.eye(3, dtype=np.float32))
            out.append('LightSource "infinite" "rgb L" [%s] "integer nsamples" [1]' % f(lt["L"]))
        else:
            raise NotImplementedError("exporter: light kind %d" % int(lt["kind"]))
    out.append("WorldEnd")
    open(path, "w").write("\n".join(out) + "\n")


def instanced_room(bvh_builder, scenes):
    """ground, wall, an area light and a point light; five transformed instances of a four-triangle pyramid object, one instance of
    a single-triangle object (no aggregate of its own, api.rs:3046), one identity instance (the quirk of primitive.rs:226-250) — the
    scene of tests/test_instancing.py with every instance transform built as Transform(m), which is what one Transform directive
    gives rs_pbrt (m_inv by Matrix4x4::inverse)"""
    T = scenes.Transform
    pyr = np.array([(-0.5, 0, -0.5), (0.5, 0, -0.5), (0.5, 0, 0.5), (-0.5, 0, 0.5), (0, 1, 0)], np.float32)
    sb = scenes.SceneBuilder()
    grey = sb.add_material(scenes.matte((0.5, 0.5, 0.5)))
    red = sb.add_material(scenes.plastic((0.6, 0.2, 0.15), (0.3, 0.3, 0.3), 0.15))
    sb.add_quad([(-5, 0, -5), (-5, 0, 5), (5, 0, 5), (5, 0, -5)], grey)
    sb.add_quad([(-5, 0, 5), (-5, 5, 5), (5, 5, 5), (5, 0, 5)], grey)
    sb.add_quad([(-1, 4, -1), (1, 4, -1), (1, 4, 1), (-1, 4, 1)], grey, emit=(10, 10, 10))
    sb.add_point_light((3, 4, -3), (30, 30, 25))
    sb.begin_object("pyr")
    sb.add_mesh(pyr, [[0, 1, 4], [1, 2, 4], [2, 3, 4], [3, 0, 4]], red)
    sb.end_object()
    sb.begin_object("one")
    sb.add_mesh(pyr[:3] + np.float32(0.1), [[0, 1, 2]], red)
    sb.end_object()
    for i in range(5):
        sb.add_instance("pyr", T((T.translate((i - 2.0, 0.2, 1.0 + 0.3 * i)) * T.rotate_y(20.0 * i + 5.0) * T.scale(0.5 + 0.1 * i, 1.0 + 0.05 * i, 0.8)).m))
    sb.add_instance("one", T(T.translate((0, 2, 0)).m))
    sb.add_instance("pyr", T.identity())
    return sb.finish(bvh_builder, instancing="reference")


def instanced_moving(bvh_builder, scenes):
    """instanced_room with MOVING instances (AnimatedTransform primitive_to_world, primitive.rs:198-265): one that slides and grows (no rotation between its
    keys: motion_bounds = the union of the keys' boxes), one that also turns (slerp; motion_bounds per corner, transform.rs:2164-2210), one whose keys are
    equal, a static one.  Every key is Transform(m) — what a `Transform [..]` directive gives rs_pbrt.  The keys hold for the whole shutter (TransformTimes 0 1,
    the file's default): per-instance key times other than the global TransformTimes cannot be written in a .pbrt file."""
    T = scenes.Transform
    pyr = np.array([(-0.5, 0, -0.5), (0.5, 0, -0.5), (0.5, 0, 0.5), (-0.5, 0, 0.5), (0, 1, 0)], np.float32)
    sb = scenes.SceneBuilder()
    grey = sb.add_material(scenes.matte((0.5, 0.5, 0.5)))
    red = sb.add_material(scenes.plastic((0.6, 0.2, 0.15), (0.3, 0.3, 0.3), 0.15))
    sb.add_quad([(-5, 0, -5), (-5, 0, 5), (5, 0, 5), (5, 0, -5)], grey)
    sb.add_quad([(-5, 0, 5), (-5, 5, 5), (5, 5, 5), (5, 0, 5)], grey)
    sb.add_quad([(-1, 4, -1), (1, 4, -1), (1, 4, 1), (-1, 4, 1)], grey, emit=(10, 10, 10))
    sb.begin_object("pyr")
    sb.add_mesh(pyr, [[0, 1, 4], [1, 2, 4], [2, 3, 4], [3, 0, 4]], red)
    sb.end_object()
    K = lambda t: T(t.m)   # noqa: E731
    sb.add_instance("pyr", K(T.translate((-2.2, 0.1, 1.0)) * T.scale(0.6, 0.8, 0.6)), K(T.translate((-1.4, 0.5, 1.6)) * T.scale(0.9, 1.3, 0.7)))
    sb.add_instance("pyr", K(T.translate((-0.3, 0.2, 0.6)) * T.rotate_y(10.0)), K(T.translate((0.2, 0.2, 1.0)) * T.rotate_y(75.0) * T.scale(1.0, 1.2, 1.0)))
    same = K(T.translate((1.2, 0.1, 1.4)) * T.rotate_y(30.0))
    sb.add_instance("pyr", same, T(same.m))
    sb.add_instance("pyr", K(T.translate((2.4, 0.0, 2.2)) * T.scale(0.7, 0.7, 0.7)))
    return sb.finish(bvh_builder, instancing="reference")


def sky_blocks(bvh_builder, scenes):
    """an open scene under a constant sky (InfiniteAreaLight: le on escape, importance sampling of a 1x1 map, the world radius) plus a
    point light; two boxes on a ground plane behind a screen perforated by an alpha mask (a float dots texture that is exactly 0 inside
    the dots: Triangle::intersect / intersect_p drop those hits, triangle.rs:313-330, :593-655)"""
    sb = scenes.SceneBuilder()
    grey = sb.add_material(scenes.matte((0.5, 0.5, 0.5)))
    blue = sb.add_material(scenes.plastic((0.2, 0.3, 0.6), (0.3, 0.3, 0.3), 0.1))
    sb.add_quad([(-200, 0, -400), (-200, 0, 900), (800, 0, 900), (800, 0, -400)], grey)
    sb.add_box((130, 0, 65), (290, 165, 230), blue)
    sb.add_box((265, 0, 296), (430, 330, 456), grey)
    holes = sb.dots_texture(sb.constant_texture(1.0), sb.constant_texture(0.0), su=6.0, sv=6.0)
    sb.add_quad([(60, 0, 20), (500, 0, 20), (500, 300, 20), (60, 300, 20)], grey, UV=[[0, 0], [1, 0], [1, 1], [0, 1]], alpha=holes, shadow_alpha=holes)
    sb.add_infinite_light((0.6, 0.7, 0.9))
    sb.add_point_light((278, 500, -200), (4e5, 4e5, 3.5e5))
    return sb.finish(bvh_builder)


def alpha_cutouts(bvh_builder, scenes):
    """the Cornell room with a panel and a uv-less triangle in front of the back wall whose "float imagemap" alpha / shadowalpha textures cut holes into them
    (8-bit images: exactly 0 or 1; the lookups at the alpha test have no ray differentials, so they are bilinear at level 0 whatever the filter — the form the
    library's traversal kernels evaluate in line)"""
    rng = np.random.default_rng(5)
    sb = scenes.SceneBuilder()
    white = sb.add_material(scenes.matte((0.725, 0.71, 0.68)))
    green = sb.add_material(scenes.matte((0.14, 0.45, 0.091)))
    sb.add_quad([(0, 0, 0), (0, 0, 560), (556, 0, 560), (556, 0, 0)], white)
    sb.add_quad([(0, 549, 0), (556, 549, 0), (556, 549, 560), (0, 549, 560)], white)
    sb.add_quad([(0, 0, 560), (0, 549, 560), (556, 549, 560), (556, 0, 560)], white)
    sb.add_quad([(213, 548.7, 227), (343, 548.7, 227), (343, 548.7, 332), (213, 548.7, 332)], white, emit=(17, 12, 4))
    a8 = (rng.random((16, 16)) > 0.45).astype(np.uint8) * 255
    b8 = (rng.random((8, 12)) > 0.4).astype(np.uint8) * 255
    m = sb.image_texture_u8(np.repeat(a8[:, :, None], 3, 2), channels=1, su=2.0, sv=3.0, du=0.25, dv=-0.4)
    ms = sb.image_texture_u8(np.repeat(b8[:, :, None], 3, 2), channels=1, su=1.0, sv=2.0, wrap="clamp", trilinear=True)
    sb.add_quad([(100, 60, 300), (460, 60, 300), (460, 420, 300), (100, 420, 300)], green, UV=[[0, 0], [1, 0], [1, 1], [0, 1]], alpha=m, shadow_alpha=ms)
    sb.add_mesh(np.array([(60, 300, 200), (260, 330, 220), (140, 520, 210)], np.float32), [[0, 1, 2]], green, alpha=m)
    return sb.finish(bvh_builder)


INSTANCED_CAMERA = (((0, 2.5, -6), (0, 0.5, 0), (0, 1, 0)), 40.0)


def camera_of(name, scenes):
    """(look_at, fov) of a scene of SCENES"""
    cam = SCENES[name][1]
    if cam == "CORNELL_DOCS":
        return scenes.CORNELL_DOCS_LOOK_AT, scenes.CORNELL_DOCS_FOV
    return (scenes.CORNELL_LOOK_AT, scenes.CORNELL_FOV) if cam == "CORNELL" else cam


SCENES = {
    # name: (scene factory(builder), "CORNELL" | (look_at, fov), xres, yres, spp, max_depth)
    "cornell_matte": (lambda b, s: s.cornell_box(b), "CORNELL", 64, 64, 16, 5),
    "cornell_mixed": (lambda b, s: s.cornell_box(b, "mixed"), "CORNELL", 64, 64, 16, 5),
    "cornell_rough": (lambda b, s: s.cornell_box(b, "rough"), "CORNELL", 64, 64, 16, 5),
    # VolPathIntegrator with a homogeneous medium filling the room; the four PCG-backed pixel samplers
    "cornell_fog_volpath": (lambda b, s: s.cornell_box(b, fog=s.CORNELL_FOG), "CORNELL", 64, 64, 16, 5),
    "cornell_02sequence": (lambda b, s: s.cornell_box(b, "mixed"), "CORNELL", 80, 80, 16, 5),
    "cornell_random": (lambda b, s: s.cornell_box(b, "mixed"), "CORNELL", 80, 80, 16, 5),
    "cornell_stratified": (lambda b, s: s.cornell_box(b, "mixed"), "CORNELL", 80, 80, 16, 5),
    "cornell_maxmindist": (lambda b, s: s.cornell_box(b, "mixed"), "CORNELL", 80, 80, 16, 5),
    # the texture stage: every procedural texture class, 2-D and 3-D mappings, float textures behind roughness and bump
    "cornell_procedural": (lambda b, s: s.cornell_box(b, "procedural"), "CORNELL", 64, 64, 16, 5),
    # image textures read from 8-bit PNGs written next to the scene (the generator's texels are u8 / 255, as ImageTexture::new computes them)
    "cornell_imagemap": (lambda b, s: s.cornell_box(b, "imagemap"), "CORNELL", 64, 64, 16, 5),
    # ObjectBegin / ObjectInstance: v0.9.12's behaviour (instanced hits lose their primitive, identity instances report nothing) is what
    # the fixture will record; the oracle's RSPT_INSTANCING_REFERENCE mode claims to reproduce it
    "instanced_room": (instanced_room, INSTANCED_CAMERA, 96, 72, 8, 5),
    # round 5: MOVING instances — AnimatedTransform::new's decomposition, interpolate per ray, and (in the dump's BVH node array) motion_bounds of the top-level boxes
    "instanced_moving": (instanced_moving, INSTANCED_CAMERA, 96, 72, 8, 5),
    # the other samplers / integrators that share the loop
    "cornell_halton": (lambda b, s: s.cornell_box(b, "mixed"), "CORNELL", 64, 64, 16, 5),
    # DirectLightingIntegrator (both strategies; the glass block in its two-lobe form, allow_multiple_lobes = false: the specular tree
    # of reflection + transmission) and AOIntegrator
    "cornell_directlighting": (lambda b, s: s.cornell_box(b, "mixed_two_lobes"), "CORNELL", 64, 64, 8, 5),
    "cornell_directlighting_one": (lambda b, s: s.cornell_box(b, "mixed_two_lobes"), "CORNELL", 64, 64, 8, 5),
    "cornell_ao": (lambda b, s: s.cornell_box(b), "CORNELL", 64, 64, 4, 5),
    # the material recipes the other scenes leave out: substrate, uber (opacity < 1, Kr, Kt), translucent, rough glass
    "cornell_layered": (lambda b, s: s.cornell_box(b, "layered"), "CORNELL", 64, 64, 16, 5),
    # InfiniteAreaLight (constant L) + a point light, alpha / shadowalpha masks
    "sky_blocks": (sky_blocks, "CORNELL", 64, 64, 16, 5),
    # a camera that turns and travels while the shutter is open (TransformTimes / ActiveTransform): AnimatedTransform decompose + slerp per ray,
    # with a thin lens, over the image-textured box (the differentials go through the interpolated matrix too)
    "cornell_moving_camera": (lambda b, s: s.cornell_box(b, "imagemap"), "CORNELL", 64, 64, 16, 5),
    # the scene of the reference's own documentation renders as recovered from them (scenes.cornell_box_docs, tests/test_reference_pin.py): rs_pbrt's
    # ref.png of this file should BE docs/source/cornell_box_8_pixelsamples.png (the oracle's render equals it byte for byte in 94 % of the pixels)
    "cornell_docs": (lambda b, s: s.cornell_box_docs(b), "CORNELL_DOCS", 500, 500, 8, 5),
    # round 4: a pixel filter wider than a pixel (the film stage's gather form) and image alpha masks (evaluated in line in the traversal)
    "cornell_gaussian": (lambda b, s: s.cornell_box(b, "mixed"), "CORNELL", 64, 64, 16, 5),
    "alpha_cutouts": (alpha_cutouts, "CORNELL", 64, 64, 16, 5),
}
# what make_render_desc / export take beyond the table above, per scene
EXTRA = {
    "cornell_docs": dict(mirror_x=True),
    "cornell_gaussian": dict(filter=("gaussian", (2.0, 2.0), 2.0)),
    "cornell_fog_volpath": dict(integrator="volpath"),
    "cornell_02sequence": dict(sampler="02sequence", dimensions=4),
    "cornell_random": dict(sampler="random"),
    "cornell_stratified": dict(sampler="stratified", strat=(4, 4), jitter=True, dimensions=4),
    "cornell_maxmindist": dict(sampler="maxmindist", dimensions=4),
    "cornell_halton": dict(sampler="halton"),
    "cornell_directlighting": dict(integrator="directlighting", direct_strategy="all"),
    "cornell_directlighting_one": dict(integrator="directlighting", direct_strategy="one"),
    "cornell_ao": dict(integrator="ao", ao_samples=16, ao_cos_sample=True),
    "cornell_moving_camera": dict(look_at_end=((340.0, 300.0, -760.0), (250.0, 260.0, 0.0), (0.1, 1.0, 0.0)), camera_times=(0.2, 0.9), shutter=(0.0, 1.0), lens_radius=4.0, focal_distance=1000.0),
}


def render_kwargs(name, scenes):
    """EXTRA[name] as make_render_desc takes it: a "filter" entry becomes the radius and the 16 x 16 table Film::new tabulates (film.rs:198-211)"""
    kw = dict(EXTRA.get(name, {}))
    filt = kw.pop("filter", None)
    if filt is not None:
        assert filt[0] == "gaussian"
        kw.update(filter_radius=filt[1], filter_table=scenes.gaussian_filter_table(filt[1], filt[2]))
    return kw


def main():
    from rs_pbrt_amd import abi, lib, scenes
    d = os.path.join(ROOT, "tests", "golden", "ref_scenes")
    os.makedirs(d, exist_ok=True)
    for name, (mk, cam, xres, yres, spp, depth) in SCENES.items():
        sc = mk(lib.bvh_build, scenes)
        look_at, fov = camera_of(name, scenes)
        export(sc, os.path.join(d, name + ".pbrt"), look_at, fov, xres, yres, spp, depth, **EXTRA.get(name, {}))
    rng = np.random.default_rng(1234)   # the stage-level fixture: rays through the Cornell box, RAY_DT records
    rays = np.zeros(4096, abi.RAY_DT)
    rays["o"] = rng.uniform(20, 530, (4096, 3)).astype(np.float32)
    v = rng.normal(size=(4096, 3))
    rays["d"] = (v / np.linalg.norm(v, axis=1)[:, None]).astype(np.float32)
    rays["t_max"] = np.inf
    rays["id"] = np.arange(4096, dtype=np.uint32)
    rays.tofile(os.path.join(d, "rays.bin"))
    print("wrote", sorted(os.listdir(d)))


if __name__ == "__main__":
    main()
